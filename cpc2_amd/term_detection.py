"""Query-by-example spoken term detection on the MI355X (csrc/sdtw.hip, cpc_sdtw).

Given a spoken query and a collection of documents, rank the documents by whether they contain the query, from the features
alone: a SUBSEQUENCE DTW in which the query may start and end anywhere inside the document.  The reference has no such task.

The definition (include/cpc2_hip.h has the same text).  For a query of n >= 1 frames and a document of m >= 1 frames, d[i][j] is
the frame distance of cpc_abx_dtw (cosine: acos(clamp(<q_i, x_j>, -1, 1)) / pi on rows the caller normalised; euclidian:
||q_i - x_j||; f32, k-ordered fma chain).  Every cell carries (cost, length, start):
    row 0:           cost = d[0][j], length = 1, start = j            (the start is free: no left predecessor)
    i > 0, j = 0:    the predecessor is up
    otherwise:       the predecessor of smallest cost among diag (i-1, j-1), left (i, j-1), up (i-1, j); ties: diag, left, up
    cost = d[i][j] + pred.cost (one f32 addition), length = pred.length + 1, start = pred.start
Detection: v[j] = cost[n-1][j] / length[n-1][j] (one f32 division); score = min_j v[j], the first j among equals; the outputs per
pair are score, start, end = j and length.  m < n is allowed (the path may go straight up).  No slope or band constraint is
applied and one detection is made per pair.  A pair whose item index or length is out of range gets NaN, -1, -1, -1.

subsequence_dtw plans the work list (plan_segments: a query's document list is split into segments of about equal numbers of
CELLS, so that a few queries against many documents still fill the device) and runs cpc_sdtw; rank orders each query's
documents; metrics turns ranks and relevance into average precision, P@10, P@N and reciprocal rank per query and their means.
There is no CPU path for the DTW: tensors must be on the GPU.
"""
import math

import numpy as np
import torch

from . import _lib

COSINE, EUCLIDIAN = 0, 1
STRIP = 64                         # query rows per strip of the kernel: longer queries need its scratch
TARGET_SEGMENTS = 4096             # segments a default plan aims at: 256 CUs x 4 workgroups x 4 turns


def distance_code(name):
    if name == "cosine":
        return COSINE
    if name == "euclidian":
        return EUCLIDIAN
    raise ValueError(f"term detection: unknown distance mode {name!r} (cosine or euclidian)")


# --------------------------------------------------------------------------- planner
def plan_segments(queries, docs, lens, exclude=None, cell_budget=None, target_segments=TARGET_SEGMENTS):
    """The kernel's work list on the host.  queries: item indices of the queries; docs: one array of document item indices for
    all queries, or one array per query; lens: the length of every item; exclude: (query item, document item) pairs left out
    (a query cut from a document is not scored against it).  Every other (query, document) pair appears exactly once, in
    the order given.  A segment holds consecutive documents of one query and at most cell_budget cells (query frames x
    document frames, summed) unless a single pair has more; by default the budget is the total over target_segments.
    Returns (seg_q [S] int32, seg_start [S + 1] int32, pair_doc [P] int32, pair_q [P] int32: the POSITION of the pair's query in
    `queries`)."""
    lens = np.asarray(lens, dtype=np.int64)
    queries = np.asarray(queries, dtype=np.int64).reshape(-1)
    shared = not (isinstance(docs, (list, tuple)) and len(docs) and not np.isscalar(docs[0]))
    excluded = {}
    for q, d in (exclude or ()):
        excluded.setdefault(int(q), set()).add(int(d))
    per_query = []
    for k, q in enumerate(queries):
        dk = np.asarray(docs if shared else docs[k], dtype=np.int64).reshape(-1)
        drop = excluded.get(int(q))
        if drop:
            dk = dk[~np.isin(dk, np.fromiter(drop, dtype=np.int64))]
        per_query.append(dk)
    if cell_budget is None:
        total = sum(int(lens[q]) * int(lens[dk].sum()) for q, dk in zip(queries, per_query))
        cell_budget = max(1, -(-total // max(1, int(target_segments))))
    cell_budget = int(cell_budget)
    if cell_budget < 1:
        raise ValueError(f"term detection: cell_budget {cell_budget} must be >= 1")
    seg_q, seg_start, n_pairs = [], [0], 0
    for q, dk in zip(queries, per_query):
        if dk.size == 0:
            continue
        cells = int(lens[q]) * lens[dk]
        ends = np.cumsum(cells)
        first, done = 0, 0                                # greedy: close a segment before the pair that would overflow it
        while first < dk.size:
            last = int(np.searchsorted(ends, done + cell_budget, side="right"))
            last = max(last, first + 1)                    # a pair larger than the budget is a segment of its own
            seg_q.append(int(q))
            n_pairs += last - first
            seg_start.append(n_pairs)
            done = int(ends[last - 1])
            first = last
    pair_doc = np.concatenate(per_query) if per_query else np.zeros(0, np.int64)
    pair_q = np.repeat(np.arange(len(queries)), [dk.size for dk in per_query])
    return (np.asarray(seg_q, dtype=np.int32), np.asarray(seg_start, dtype=np.int32), pair_doc.astype(np.int32),
            pair_q.astype(np.int32))


# --------------------------------------------------------------------------- kernel call
def check_work_list(what, frames, item_off, item_len, seg_row, seg_start, pair_col, names):
    """The checks of a run_segments (here and in term_discovery; `what` labels the messages, names = what the caller calls
    seg_row and pair_col): frames as contiguous f32 [total_frames, dp], the work list as contiguous int32 device tensors, one more
    seg_start than segments.  Returns (frames, n_seg, n_pairs)."""
    _lib.require_gpu(frames, item_off, item_len, seg_row, seg_start, pair_col)
    frames = _lib.f32c(frames)
    if frames.dim() != 2:
        raise ValueError(f"{what}: frames must be [total_frames, dp], got {tuple(frames.shape)}")
    for name, t in (("item_off", item_off), ("item_len", item_len), (names[0], seg_row), ("seg_start", seg_start),
                    (names[1], pair_col)):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise TypeError(f"{what}: {name} must be a contiguous int32 tensor")
    n_seg, n_pairs = int(seg_row.numel()), int(pair_col.numel())
    if seg_start.numel() != n_seg + 1:
        raise ValueError(f"{what}: seg_start has {seg_start.numel()} entries for {n_seg} segments")
    return frames, n_seg, n_pairs


def _call_segments(what, name, query, call, tag, head, work, sizes, params, span_width, scratch):
    """The library call of a run_segments (here and in term_discovery): `call` (the entry point `name`) on a checked work list.
    head: the arguments before item_off, the device tensor of frames or units first; work: item_off, item_len, seg_row, seg_start,
    pair_col; sizes: n_seg, n_pairs, max_len_row, max_len_col; params: the arguments between max_len_col and score.  The
    boundary-row buffer is the caller's `scratch` when it holds query(...) bytes, else the package's arena under `tag` (None for 0
    bytes).  Returns (score [P] f32, span [P, span_width] int32)."""
    dev = head[0].device
    item_off, item_len, seg_row, seg_start, pair_col = work
    n_seg, n_pairs, max_len_row, max_len_col = (int(v) for v in sizes)
    nbytes = query(n_seg, max_len_row, max_len_col)
    if scratch is None:
        scratch = _lib.scratch(nbytes, dev, tag=tag) if nbytes else None
    elif scratch.numel() * scratch.element_size() < nbytes:
        raise ValueError(f"{what}: scratch of {scratch.numel() * scratch.element_size()} bytes, {nbytes} needed")
    score = torch.empty(n_pairs, dtype=torch.float32, device=dev)
    span = torch.empty(n_pairs, span_width, dtype=torch.int32, device=dev)
    _lib.check(call(_lib.ptr(head[0]), *head[1:], _lib.ptr(item_off), _lib.ptr(item_len), int(item_len.numel()), _lib.ptr(seg_row),
                    _lib.ptr(seg_start), _lib.ptr(pair_col), n_seg, max_len_row, max_len_col, *params, _lib.ptr(score),
                    _lib.ptr(span), _lib.ptr(scratch), nbytes, _lib.stream_ptr(dev)), name)
    return score, span


def run_segments(frames, item_off, item_len, seg_q, seg_start, pair_doc, max_len_q, max_len_doc, distance, scratch=None):
    """cpc_sdtw on a given work list (device int32 tensors): (score [P] f32, span [P, 3] int32: start, end, length).  scratch:
    a device buffer of at least cpc_sdtw_scratch_bytes (default: the package's arena)."""
    frames, n_seg, n_pairs = check_work_list("term detection", frames, item_off, item_len, seg_q, seg_start, pair_doc,
                                             ("seg_q", "pair_doc"))
    lib = _lib.load()
    return _call_segments("term detection", "cpc_sdtw", lib.cpc_sdtw_scratch_bytes, lib.cpc_sdtw, "sdtw", (frames, frames.size(1)),
                          (item_off, item_len, seg_q, seg_start, pair_doc), (n_seg, n_pairs, max_len_q, max_len_doc),
                          (int(distance),), 3, scratch)


def _subsequence(run, data, item_len, queries, docs, exclude, lens_host, cell_budget, target_segments):
    """What subsequence_dtw and subsequence_dtw_units do once `data` (frames or units) is checked: the plan on the host, its upload,
    and run(seg_q, seg_start, pair_doc, max_len_q, max_len_doc), the run_segments of the kind."""
    lens = np.asarray(item_len.cpu().numpy() if lens_host is None else lens_host, dtype=np.int64)
    seg_q, seg_start, pair_doc, pair_q = plan_segments(queries, docs, lens, exclude, cell_budget, target_segments)
    dev = data.device
    if pair_doc.size == 0:
        return (torch.empty(0, dtype=torch.float32, device=dev), torch.empty(0, 3, dtype=torch.int32, device=dev), pair_q,
                pair_doc)
    max_len_q = max(1, int(lens[seg_q].max()))
    max_len_doc = max(1, int(lens[pair_doc].max()))
    score, span = run(torch.from_numpy(seg_q).to(dev), torch.from_numpy(seg_start).to(dev), torch.from_numpy(pair_doc).to(dev),
                      max_len_q, max_len_doc)
    return score, span, pair_q, pair_doc


def subsequence_dtw(frames, item_off, item_len, queries, docs, distance, exclude=None, lens_host=None, cell_budget=None,
                    target_segments=TARGET_SEGMENTS):
    """Subsequence DTW of every query against its documents.  frames [total_frames, dp] f32 (dp a multiple of 4, padding
    columns zero, rows normalised by the caller for the cosine distance), item_off / item_len int32: the device layout of
    ABXFeatureLoader.device_frames.  queries, docs, exclude, cell_budget: see plan_segments.  distance: COSINE / EUCLIDIAN or
    their names.  Returns (score [P] f32, span [P, 3] int32 (start, end, length), pair_q [P], pair_doc [P]): the first two on the
    device, the pair lists as int32 numpy arrays (pair_q: position in `queries`)."""
    _lib.require_gpu(frames, item_off, item_len)
    if isinstance(distance, str):
        distance = distance_code(distance)
    return _subsequence(lambda *work: run_segments(frames, item_off, item_len, *work, distance), frames, item_len, queries,
                        docs, exclude, lens_host, cell_budget, target_segments)


# --------------------------------------------------------------------------- quantized units (csrc/sdtw_units.hip)
def check_unit_work_list(what, units, item_off, item_len, seg_row, seg_start, pair_col, names):
    """check_work_list for items of unit ids (here and in term_discovery): units as a contiguous int32 device tensor
    [total_frames]; anything else is a TypeError that names the argument.  Returns (n_seg, n_pairs)."""
    for name, t in (("units", units), ("item_off", item_off), ("item_len", item_len), (names[0], seg_row), ("seg_start", seg_start),
                    (names[1], pair_col)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or not t.is_contiguous():
            raise TypeError(f"{what}: {name} must be a contiguous int32 tensor")
    if units.dim() != 1:
        raise TypeError(f"{what}: units must be [total_frames], got {tuple(units.shape)}")
    _lib.require_gpu(units, item_off, item_len, seg_row, seg_start, pair_col)
    n_seg, n_pairs = int(seg_row.numel()), int(pair_col.numel())
    if seg_start.numel() != n_seg + 1:
        raise ValueError(f"{what}: seg_start has {seg_start.numel()} entries for {n_seg} segments")
    return n_seg, n_pairs


def _check_units(what, units, item_off, item_len):
    """The input check of subsequence_dtw_units and term_discovery.local_alignment_units."""
    if not isinstance(units, torch.Tensor) or units.dtype != torch.int32 or not units.is_contiguous() or units.dim() != 1:
        raise TypeError(f"{what}: units must be a contiguous int32 tensor [total_frames]")
    _lib.require_gpu(units, item_off, item_len)


def run_segments_units(units, item_off, item_len, seg_q, seg_start, pair_doc, max_len_q, max_len_doc, d_same, d_diff, scratch=None):
    """cpc_sdtw_units on a given work list (device int32 tensors): run_segments with the frames replaced by unit ids
    [total_frames] int32 and the distance by its two values (d_same between equal units, d_diff between different ones;
    abx_group_computation.unit_frame_distances makes them).  scratch: at least cpc_sdtw_units_scratch_bytes."""
    n_seg, n_pairs = check_unit_work_list("term detection on units", units, item_off, item_len, seg_q, seg_start, pair_doc,
                                          ("seg_q", "pair_doc"))
    lib = _lib.load()
    return _call_segments("term detection on units", "cpc_sdtw_units", lib.cpc_sdtw_units_scratch_bytes, lib.cpc_sdtw_units,
                          "sdtw_units", (units,), (item_off, item_len, seg_q, seg_start, pair_doc),
                          (n_seg, n_pairs, max_len_q, max_len_doc), (float(d_same), float(d_diff)), 3, scratch)


def subsequence_dtw_units(units, item_off, item_len, queries, docs, d_same, d_diff, exclude=None, lens_host=None, cell_budget=None,
                          target_segments=TARGET_SEGMENTS):
    """subsequence_dtw on items of unit ids: units [total_frames] int32 on the device, d_same / d_diff the frame distance between
    equal / different units.  The same plan and the same returns.  target_segments keeps the dense default of 4096: a workgroup
    serves four pairs at once here, but a segment is still what a workgroup takes, and tools/term_units_bench.py does not vary
    it, so there is no measured reason for another value."""
    _check_units("term detection on units", units, item_off, item_len)
    return _subsequence(lambda *work: run_segments_units(units, item_off, item_len, *work, d_same, d_diff), units, item_len,
                        queries, docs, exclude, lens_host, cell_budget, target_segments)


# --------------------------------------------------------------------------- ranking and scores
def rank(score, pair_q, pair_doc):
    """Ranks per query: ascending score, ties by ascending document index, NaN last.  score [P] (any device), pair_q and
    pair_doc [P] integers.  Returns (order, ranks) as int64 numpy arrays: order lists the pairs query by query, best first;
    ranks[p] is the 1-based rank of pair p among the pairs of its query.  Three stable sorts where the scores are."""
    score = torch.as_tensor(score)
    dev = score.device
    q = torch.as_tensor(np.asarray(pair_q, dtype=np.int64)).to(dev)
    d = torch.as_tensor(np.asarray(pair_doc, dtype=np.int64)).to(dev)
    order = torch.sort(d, stable=True)[1]
    order = order[torch.sort(score[order], stable=True)[1]]              # torch sorts NaN behind every number
    order = order[torch.sort(q[order], stable=True)[1]]
    q_sorted = q[order]
    pos = torch.arange(order.numel(), device=dev)
    is_first = torch.ones_like(q_sorted, dtype=torch.bool)
    is_first[1:] = q_sorted[1:] != q_sorted[:-1]
    first_pos = torch.cummax(torch.where(is_first, pos, torch.zeros_like(pos)), 0)[0] if order.numel() else pos
    ranks = torch.empty_like(order)
    ranks[order] = pos - first_pos + 1
    return order.cpu().numpy(), ranks.cpu().numpy()


def metrics(ranks, pair_q, relevant, n_queries, names=None):
    """Scores from integer ranks.  ranks [P]: 1-based rank of every pair within its query (rank); pair_q [P]: its query;
    relevant [P]: whether the document contains the query.  Per query with R >= 1 relevant candidates at ranks
    r_1 < ... < r_R:  AP = (1 / R) sum_k k / r_k,  P@10 = #{r_k <= 10} / 10,  P@N = #{r_k <= R} / R,  RR = 1 / r_1.
    MAP, mean P@10, mean P@N and MRR are taken over those queries, on the host in float64 with math.fsum.  Queries without a
    relevant candidate are counted and listed (by `names` when given), not averaged."""
    ranks = np.asarray(ranks, dtype=np.int64)
    pair_q = np.asarray(pair_q, dtype=np.int64)
    relevant = np.asarray(relevant, dtype=bool)
    by_query = [[] for _ in range(int(n_queries))]
    for r, q in zip(ranks[relevant].tolist(), pair_q[relevant].tolist()):
        by_query[q].append(r)
    per_query, unscored = {}, []
    for q, rs in enumerate(by_query):
        name = names[q] if names is not None else q
        if not rs:
            unscored.append(name)
            continue
        rs.sort()
        n_rel = len(rs)
        per_query[name] = {"n_relevant": n_rel,
                           "ap": math.fsum((k + 1) / r for k, r in enumerate(rs)) / n_rel,
                           "p_at_10": sum(r <= 10 for r in rs) / 10,
                           "p_at_n": sum(r <= n_rel for r in rs) / n_rel,
                           "rr": 1 / rs[0]}
    n = len(per_query)

    def mean(key):
        return math.fsum(v[key] for v in per_query.values()) / n if n else float("nan")

    return {"map": mean("ap"), "p_at_10": mean("p_at_10"), "p_at_n": mean("p_at_n"), "mrr": mean("rr"), "n_queries": int(n_queries),
            "n_scored": n, "n_without_relevant": len(unscored), "without_relevant": unscored, "per_query": per_query}
