"""Term detection and term discovery on quantized units on the device (csrc/sdtw_units.hip, csrc/lalign_units.hip; DESIGN.md
section 29).  The statement is tests/term_units_oracle.py: the f32 programs of the dense kernels' definitions on the two-valued
distance matrix.  The distances are given, not computed, so the kernels are held to EQUALITY on every case, ties included: the
score as a bit pattern and every span integer."""
import json

import numpy as np
import pytest
import torch

from cpc2_amd import _lib
from cpc2_amd import term_detection as td
from cpc2_amd import term_discovery as tdisc
from cpc2_amd.eval import term_detection as detection_tool
from cpc2_amd.eval import term_discovery as discovery_tool
from cpc2_amd.eval.ABX import abx_iterators as abx_it
from tests import term_units_oracle as U

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CAP = 2048                                                    # workgroups per launch
POISON = 0                                                    # the id between items: a real unit of every alphabet


# --------------------------------------------------------------------------- inputs and calls
def _pack(items, gap=0):
    """Items as one int32 buffer with `gap` frames of POISON before, between and behind them."""
    parts, offs, lens, at = [], [], [], 0
    for v in items:
        if gap:
            parts.append(np.full(gap, POISON, dtype=np.int32))
            at += gap
        parts.append(np.asarray(v, dtype=np.int32))
        offs.append(at)
        lens.append(len(v))
        at += len(v)
    parts.append(np.full(max(gap, 1), POISON, dtype=np.int32))
    units = torch.from_numpy(np.concatenate(parts)).to(DEV)
    return units, torch.tensor(offs, dtype=torch.int32, device=DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), np.asarray(lens)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _run(kind, packed, plan, config, scratch_fill=None):
    """One launch of cpc_sdtw_units ("sdtw") or cpc_local_align_units ("align") on a work list: (score [P] f32, span [P, 3 | 5])
    on the host."""
    units, off, lens, lens_host = packed
    seg_row, seg_start, pair_col = (np.asarray(a) for a in plan[:3])
    (d_same, d_diff), (theta, gamma) = U.CONFIGS[config] if isinstance(config, int) else config
    max_row, max_col = int(lens_host[seg_row].max()), int(lens_host[pair_col].max())
    scratch = None
    if scratch_fill is not None:
        query = _lib.load().cpc_sdtw_units_scratch_bytes if kind == "sdtw" else _lib.load().cpc_local_align_units_scratch_bytes
        scratch = torch.full((max(query(len(seg_row), max_row, max_col), 1),), scratch_fill, dtype=torch.uint8, device=DEV)
    if kind == "sdtw":
        score, span = td.run_segments_units(units, off, lens, _dev(seg_row), _dev(seg_start), _dev(pair_col), max_row, max_col, d_same,
                                            d_diff, scratch=scratch)
    else:
        score, span = tdisc.run_segments_units(units, off, lens, _dev(seg_row), _dev(seg_start), _dev(pair_col), max_row, max_col,
                                               d_same, d_diff, theta, gamma, scratch=scratch)
    return score.cpu().numpy(), span.cpu().numpy()


def _plan_of_pairs(pairs):
    """One segment per run of consecutive pairs with the same row item: (seg_row, seg_start, pair_col)."""
    seg_row, seg_start = [], [0]
    for k, (a, _) in enumerate(pairs):
        if k and a == pairs[k - 1][0]:
            seg_start[-1] = k + 1
        else:
            seg_row.append(a)
            seg_start.append(k + 1)
    return np.asarray(seg_row, np.int32), np.asarray(seg_start, np.int32), np.asarray([b for _, b in pairs], np.int32)


def _want(kind, items, pairs, config):
    (d_same, d_diff), (theta, gamma) = U.CONFIGS[config] if isinstance(config, int) else config
    if kind == "sdtw":
        return [U.sdtw_units(items[a], items[b], d_same, d_diff) for a, b in pairs]
    return [U.local_align_units(items[a], items[b], d_same, d_diff, theta, gamma) for a, b in pairs]


def _assert_equal(kind, score, span, want, what=""):
    assert len(score) == len(want)
    for p, w in enumerate(want):
        ints = (w[1], w[2], w[3]) if kind == "sdtw" else w[1]
        print(what, kind, p, float(score[p]), tuple(int(x) for x in span[p]), "statement", float(w[0]), tuple(ints))
        assert U.same_bits(score[p], w[0]) and tuple(int(x) for x in span[p]) == tuple(ints), (what, p)


# --------------------------------------------------------------------------- 1. equality with the f32 statement
@pytest.mark.parametrize("config", range(len(U.CONFIGS)))
@pytest.mark.parametrize("kind", ["sdtw", "align"])
def test_equals_the_f32_statement(kind, config):
    """Row items of 1 .. 200 frames (one to four strips) against column items of 1 .. 257 (across the refills of the column
    register; 64 rows against 10 columns, where the second refill holds nothing in range; m < n), in alphabets of 2, 8 and 50
    units drawn in runs of 1 .. 5, and a column item over a disjoint alphabet."""
    items, pairs = U.family()
    want = U.family_sdtw(config) if kind == "sdtw" else U.family_align(config)
    lengths = {(len(items[a]), len(items[b])) for a, b in pairs}
    assert (64, 10) in lengths and (200, 5) in lengths and (65, 257) in lengths
    score, span = _run(kind, _pack(items), _plan_of_pairs(pairs), config)
    _assert_equal(kind, score, span, want)
    if kind == "sdtw":                                          # the free ends are used: a match inside the document
        assert any(w[1] > 0 and w[2] != len(items[b]) - 1 for w, (_, b) in zip(want, pairs))
    else:
        assert any(w[1][4] > 64 for w in want)                  # a match longer than a strip
        disjoint = [w for w, (_, b) in zip(want, pairs) if b == len(items) - 1]
        assert len(disjoint) == len(U.ROW_LENGTHS) and all(float(w[0]) == 0.0 and w[1] == (-1,) * 5 for w in disjoint)


# --------------------------------------------------------------------------- 2. the unit path equals the dense path
def _one_hot(items, n_units, cosine):
    """The one-hot expansion of the items as the dense tools hold it: rows through normalize_with_singularity for the cosine
    distance (which appends its column), plain for the euclidian; [total, dp] f32 with dp a multiple of 4, padding columns zero."""
    flat = np.concatenate(items)
    rows = torch.zeros(len(flat), n_units, dtype=torch.float32)
    rows[torch.arange(len(flat)), torch.from_numpy(flat.astype(np.int64))] = 1
    if cosine:
        rows = abx_it.normalize_with_singularity(rows)
    frames = torch.zeros(len(flat), -(-rows.size(1) // 4) * 4, dtype=torch.float32)
    frames[:, :rows.size(1)] = rows
    return frames.to(DEV)


@pytest.mark.parametrize("distance", ["cosine", "euclidian"])
def test_dense_distance_of_one_hot_rows_is_the_unit_distance(distance):
    """What the comparison below stands on, as a check of its own (DESIGN.md 7.1 records it for cpc_abx_dtw): the dense kernels'
    distance of two equal / two different one-hot rows is exactly d_same / d_diff of unit_frame_distances."""
    d_same, d_diff = detection_tool.unit_distances(distance)
    assert (d_same, d_diff) == ((0.0, 0.5) if distance == "cosine" else (0.0, U.SQRT2))
    for n_units in U.ALPHABETS:
        ids = (0, 1, n_units - 1)
        items = [np.array([u], dtype=np.int32) for u in ids]
        frames = _one_hot(items, n_units, distance == "cosine")
        off = torch.arange(3, dtype=torch.int32, device=DEV)
        lens = torch.ones(3, dtype=torch.int32, device=DEV)
        # a query of one frame in a document of one frame: the score is the frame distance
        seg_q, seg_start, pair_doc = _dev([0, 1, 2]), _dev([0, 3, 6, 9]), _dev([0, 1, 2] * 3)
        score, _ = td.run_segments(frames, off, lens, seg_q, seg_start, pair_doc, 1, 1, td.distance_code(distance))
        score = score.cpu().numpy().reshape(3, 3)
        for a in range(3):
            for b in range(3):
                assert U.same_bits(score[a, b], d_same if ids[a] == ids[b] else d_diff), (n_units, a, b, float(score[a, b]))


@pytest.mark.parametrize("distance", ["cosine", "euclidian"])
@pytest.mark.parametrize("n_units", U.ALPHABETS)
def test_unit_path_equals_dense_path(distance, n_units):
    rng = np.random.default_rng(100 + n_units)
    shapes = ((1, 1), (2, 63), (64, 10), (65, 130), (129, 257), (200, 65))
    items = [U.draw_units(rng, n, n_units) for n, _ in shapes] + [U.draw_units(rng, m, n_units) for _, m in shapes]
    pairs = [(k, len(shapes) + k) for k in range(len(shapes))]
    plan = _plan_of_pairs(pairs)
    d_same, d_diff = detection_tool.unit_distances(distance)
    config = ((d_same, d_diff), (0.25, 0.125))
    packed = _pack(items)
    frames = _one_hot(items, n_units, distance == "cosine")
    _, off, lens, lens_host = packed
    seg_row, seg_start, pair_col = (_dev(a) for a in plan)
    max_row, max_col = int(lens_host[plan[0]].max()), int(lens_host[plan[2]].max())
    code = td.distance_code(distance)
    for kind in ("sdtw", "align"):
        score_u, span_u = _run(kind, packed, plan, config)
        if kind == "sdtw":
            score_d, span_d = td.run_segments(frames, off, lens, seg_row, seg_start, pair_col, max_row, max_col, code)
        else:
            score_d, span_d = tdisc.run_segments(frames, off, lens, seg_row, seg_start, pair_col, max_row, max_col, code, 0.25, 0.125)
        score_d, span_d = score_d.cpu().numpy(), span_d.cpu().numpy()
        print(kind, distance, n_units, score_u, score_d)
        assert score_u.tobytes() == score_d.tobytes() and np.array_equal(span_u, span_d), kind
        _assert_equal(kind, score_u, span_u, _want(kind, items, pairs, config))


# --------------------------------------------------------------------------- 3. work lists
@pytest.mark.parametrize("kind", ["sdtw", "align"])
def test_work_lists_scratch_gaps_and_repeats_give_the_same_bits(kind):
    rng = np.random.default_rng(33)
    rows = [U.draw_units(rng, n, 8) for n in (3, 64, 65, 150)]
    cols = [U.draw_units(rng, m, 8) for m in (1, 9, 63, 64, 65, 70, 130, 131, 200)]
    items = cols + rows
    nc = len(cols)
    packed = _pack(items)
    lens_host = packed[3]
    row_ids, col_ids = np.arange(nc, nc + len(rows)), np.arange(nc)
    pairs = [(int(a), int(b)) for a in row_ids for b in col_ids]
    want = _want(kind, items, pairs, 0)
    per_row = td.plan_segments(row_ids, col_ids, lens_host, cell_budget=10 ** 9)
    per_pair = td.plan_segments(row_ids, col_ids, lens_host, cell_budget=1)
    default = td.plan_segments(row_ids, col_ids, lens_host, target_segments=7)
    assert len(per_row[0]) == len(rows) and len(per_pair[0]) == len(pairs) and len(rows) < len(default[0]) < len(pairs)
    base = _run(kind, packed, per_row, 0)
    _assert_equal(kind, *base, want, "one segment per row item")
    # a segment of 9 pairs: round robin over four waves with a tail; below, segments of 1, 3, 4 and 5 pairs
    for name, plan, fill in (("one segment per pair", per_pair, None), ("planned", default, None), ("scratch 0x00", per_row, 0x00),
                             ("scratch 0xFF", per_row, 0xFF), ("again", per_row, None)):
        score, span = _run(kind, packed, plan, 0, scratch_fill=fill)
        assert score.tobytes() == base[0].tobytes() and np.array_equal(span, base[1]), name
    long_row = int(row_ids[-1])
    ragged = [(long_row, int(b)) for b in (6, 0, 7, 2, 8, 1, 3, 4, 5, 6, 7, 8, 0)]
    ragged_plan = (np.full(4, long_row, np.int32), np.asarray([0, 1, 4, 8, 13], np.int32), np.asarray([b for _, b in ragged], np.int32))
    _assert_equal(kind, *_run(kind, packed, ragged_plan, 0, scratch_fill=0xFF), _want(kind, items, ragged, 0), "segments of 1, 3, 4, 5 pairs")
    # gaps of a unit that occurs in the items: a read outside an item would change a result
    assert all((np.asarray(v) == POISON).any() for v in items if len(v) >= 60)
    score, span = _run(kind, _pack(items, gap=67), per_row, 0)
    assert score.tobytes() == base[0].tobytes() and np.array_equal(span, base[1]), "gaps"


@pytest.mark.parametrize("kind", ["sdtw", "align"])
def test_every_output_is_written_and_nothing_else(kind):
    rng = np.random.default_rng(34)
    items = [U.draw_units(rng, n, 8) for n in (70, 5, 40, 66, 130)]
    units, off, lens, _ = _pack(items)
    pairs = [(0, b) for b in (1, 2, 3, 4, 1, 2)] + [(1, b) for b in (0, 2, 3)]
    seg_row, seg_start, pair_col = _plan_of_pairs(pairs)
    lists = [_dev(seg_row), _dev(seg_start), _dev(pair_col)]                     # held until the kernel has run
    width = 3 if kind == "sdtw" else 5
    n_pairs, pad = len(pairs), 7
    score = torch.full((n_pairs + pad,), -777.0, dtype=torch.float32, device=DEV)
    span = torch.full((n_pairs + pad, width), -777, dtype=torch.int32, device=DEV)
    lib = _lib.load()
    (d_same, d_diff), (theta, gamma) = U.CONFIGS[0]
    if kind == "sdtw":
        nbytes = lib.cpc_sdtw_units_scratch_bytes(len(seg_row), 70, 130)
        scratch = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
        status = lib.cpc_sdtw_units(_lib.ptr(units), _lib.ptr(off), _lib.ptr(lens), len(items), _lib.ptr(lists[0]),
                                    _lib.ptr(lists[1]), _lib.ptr(lists[2]), len(seg_row), 70, 130, d_same, d_diff,
                                    _lib.ptr(score), _lib.ptr(span), _lib.ptr(scratch), nbytes, _lib.stream_ptr(DEV))
    else:
        nbytes = lib.cpc_local_align_units_scratch_bytes(len(seg_row), 70, 130)
        scratch = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
        status = lib.cpc_local_align_units(_lib.ptr(units), _lib.ptr(off), _lib.ptr(lens), len(items), _lib.ptr(lists[0]),
                                           _lib.ptr(lists[1]), _lib.ptr(lists[2]), len(seg_row), 70, 130, d_same, d_diff,
                                           theta, gamma, _lib.ptr(score), _lib.ptr(span), _lib.ptr(scratch), nbytes, _lib.stream_ptr(DEV))
    _lib.check(status, kind)
    torch.cuda.synchronize()
    assert nbytes == U.scratch_bytes(len(seg_row), 70, 130) > 0
    score, span = score.cpu().numpy(), span.cpu().numpy()
    assert (score[n_pairs:] == -777.0).all() and (span[n_pairs:] == -777).all()
    _assert_equal(kind, score[:n_pairs], span[:n_pairs], _want(kind, items, pairs, 0))


# --------------------------------------------------------------------------- 4. more segments than the grid cap
@pytest.mark.parametrize("n", [3, 65])
@pytest.mark.parametrize("kind", ["sdtw", "align"])
def test_more_segments_than_the_grid_cap(kind, n):
    """2 * 2048 + 3 segments of one pair each: every workgroup takes two or three segments.  At 65 rows its waves' boundary rows are
    reused from segment to segment and hold 0xFF before the launch."""
    rng = np.random.default_rng(44 + n)
    rows = [U.draw_units(rng, k, 3) for k in ((1, 2, 3, 3, 2, 1, 3) if n == 3 else (65,) * 7)]
    cols = [U.draw_units(rng, k, 3) for k in (1, 2, 3, 3, 1)]
    items = rows + cols
    n_seg = 2 * CAP + 3
    seg_row = rng.integers(0, len(rows), n_seg)
    pair_col = rng.integers(len(rows), len(items), n_seg)
    plan = (seg_row.astype(np.int32), np.arange(n_seg + 1, dtype=np.int32), pair_col.astype(np.int32))
    query = _lib.load().cpc_sdtw_units_scratch_bytes if kind == "sdtw" else _lib.load().cpc_local_align_units_scratch_bytes
    assert query(n_seg, n, 3) == (0 if n == 3 else CAP * 4 * 2 * 12 * 3)
    score, span = _run(kind, _pack(items), plan, 0, scratch_fill=0xFF)
    table = {}
    for a in range(len(rows)):
        for b in range(len(rows), len(items)):
            table[(a, b)] = _want(kind, items, [(a, b)], 0)[0]
    for p in range(n_seg):
        w = table[(int(seg_row[p]), int(pair_col[p]))]
        ints = (w[1], w[2], w[3]) if kind == "sdtw" else w[1]
        assert U.same_bits(score[p], w[0]) and tuple(int(x) for x in span[p]) == tuple(ints), p


# --------------------------------------------------------------------------- 5. pairs of one wave, one after the other
@pytest.mark.parametrize("kind", ["sdtw", "align"])
def test_nothing_leaks_from_a_pair_to_the_wave_s_next(kind):
    """Pairs p and p + 4 of a segment are one wave's: a three-strip pair with long matches, then a short column item that shares no
    unit with the row item."""
    rng = np.random.default_rng(55)
    row = U.draw_units(rng, 150, 4)
    long_col = np.concatenate([U.draw_units(rng, 20, 4), row, U.draw_units(rng, 20, 4)])
    short = U.draw_units(rng, 3, 4) + U.DISJOINT
    items = [row, long_col, short, U.draw_units(rng, 30, 4)]
    pairs = [(0, 1), (0, 3), (0, 3), (0, 3), (0, 2), (0, 2), (0, 1), (0, 1), (0, 2)]
    want = _want(kind, items, pairs, 0)
    score, span = _run(kind, _pack(items), _plan_of_pairs(pairs), 0, scratch_fill=0xFF)
    _assert_equal(kind, score, span, want)
    if kind == "align":
        assert float(want[0][0]) >= 150 * 0.25 and float(score[4]) == 0.0 and (span[4] == -1).all() and (span[8] == -1).all()
    else:
        assert float(want[0][0]) == 0.0 and float(score[4]) == 0.5 and tuple(span[4]) == (0, 0, 150)


# --------------------------------------------------------------------------- 6. uncomputable pairs and refusals
@pytest.mark.parametrize("kind", ["sdtw", "align"])
def test_uncomputable_pairs_and_refusals(kind):
    rng = np.random.default_rng(66)
    items = [U.draw_units(rng, n, 8) for n in (5, 70, 9, 80)]
    units, off, lens, _ = _pack(items)
    lens_zero = torch.cat([lens, torch.zeros(1, dtype=torch.int32, device=DEV)])       # item 4: no frame
    off_zero = torch.cat([off, torch.zeros(1, dtype=torch.int32, device=DEV)])
    # segments: row item 0 (5 frames), 1 (70 frames), 5 = n_items (out of range), -1, 4 (empty), 3 (80 frames: longer than 70)
    seg_row = _dev([0, 1, 5, -1, 4, 3])
    seg_start = _dev([0, 4, 9, 10, 11, 12, 13])
    pair_col = _dev([2, -1, 3, 4, 2, 5, 1, 0, 3, 0, 0, 0, 0])
    (d_same, d_diff), (theta, gamma) = U.CONFIGS[0]
    width = 3 if kind == "sdtw" else 5

    def run(max_col):
        if kind == "sdtw":
            return td.run_segments_units(units, off_zero, lens_zero, seg_row, seg_start, pair_col, 70, max_col, d_same, d_diff)
        return tdisc.run_segments_units(units, off_zero, lens_zero, seg_row, seg_start, pair_col, 70, max_col, d_same, d_diff, theta, gamma)

    def check_edges(max_col=80):
        score, span = (t.cpu().numpy() for t in run(max_col))
        nan = [1, 3, 5, 9, 10, 11, 12]          # index -1, empty column item, index n_items, rows: n_items, -1, empty, too long
        ok = {0: (0, 2), 2: (0, 3), 4: (1, 2), 6: (1, 1), 7: (1, 0), 8: (1, 3)}
        if max_col < 80:                        # a column item longer than the maximum given
            nan += [2, 8]
            del ok[2], ok[8]
        assert np.isnan(score[nan]).all() and (span[nan] == -1).all()
        pairs = list(ok.values())
        _assert_equal(kind, score[list(ok)], span[list(ok)], _want(kind, items, pairs, 0))

    check_edges()
    check_edges(max_col=79)

    lib = _lib.load()
    one = torch.zeros(16, dtype=torch.int32, device=DEV)
    out_score = torch.full((4,), 77.0, dtype=torch.float32, device=DEV)
    out_span = torch.full((4, width), 77, dtype=torch.int32, device=DEV)
    small = torch.zeros(64, dtype=torch.uint8, device=DEV)
    label = "sdtw_units" if kind == "sdtw" else "local_align_units"

    def call(units=one, n_items=1, n_seg=1, max_row=4, max_col=4, d_same=0.0, d_diff=0.5, theta=0.25, gamma=0.125, score=out_score,
             span=out_span, seg_row=one, item_off=one, scratch=None, scratch_bytes=0):
        head = (_lib.ptr(units), _lib.ptr(item_off), _lib.ptr(one), n_items, _lib.ptr(seg_row), _lib.ptr(one), _lib.ptr(one), n_seg,
                max_row, max_col, d_same, d_diff)
        tail = (_lib.ptr(score), _lib.ptr(span), _lib.ptr(scratch), scratch_bytes, _lib.stream_ptr(DEV))
        if kind == "sdtw":
            return lib.cpc_sdtw_units(*head, *tail)
        return lib.cpc_local_align_units(*head, theta, gamma, *tail)

    inf, nan = float("inf"), float("nan")
    workspace = -1 if kind == "sdtw" else -3                     # as the dense siblings: CPC_ERR_INVALID / CPC_ERR_WORKSPACE
    refusals = [({"units": None}, "null buffer", -1), ({"score": None}, "null buffer", -1), ({"span": None}, "null buffer", -1),
                ({"seg_row": None}, "null buffer", -1), ({"item_off": None}, "null buffer", -1),
                ({"d_same": nan}, "must not be NaN", -1), ({"d_diff": nan}, "must not be NaN", -1),
                ({"n_items": 0}, "bad sizes", -1), ({"n_seg": -1}, "bad sizes", -1), ({"max_col": 0}, "bad sizes", -1),
                ({"max_row": 0}, "bad sizes", -1), ({"max_row": -3}, "bad sizes", -1),
                ({"max_row": 65}, "scratch", workspace), ({"max_row": 65, "scratch": small, "scratch_bytes": 64}, "scratch", workspace)]
    if kind == "align":
        refusals += [({"max_row": 32768}, "at most 32767", -1), ({"max_col": 32768}, "at most 32767", -1),
                     ({"theta": 0.0}, "theta", -1), ({"theta": -0.25}, "theta", -1), ({"theta": nan}, "theta", -1),
                     ({"theta": inf}, "theta", -1), ({"gamma": -0.125}, "gamma", -1), ({"gamma": nan}, "gamma", -1),
                     ({"gamma": inf}, "gamma", -1)]
    for kwargs, word, status in refusals:
        got = call(**kwargs)
        assert got == status, (kwargs, got)
        message = lib.cpc_last_error().decode()
        assert message.startswith(label + ":") and word in message, (kwargs, message)
        with pytest.raises(ValueError if status == -1 else RuntimeError, match=word):
            _lib.check(got, label)
    assert call(n_seg=0) == 0                                    # nothing to do: OK, and nothing written
    assert call(gamma=0.0, n_seg=0) == 0
    assert call(d_diff=inf, n_seg=0) == 0                        # only NaN distances are refused
    torch.cuda.synchronize()
    assert (out_score == 77.0).all() and (out_span == 77).all()  # every refusal left the outputs untouched
    check_edges()                                                # a refusal leaves the next valid call intact
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        run_cpu = td.run_segments_units if kind == "sdtw" else tdisc.run_segments_units
        run_cpu(units.cpu(), off, lens, seg_row, seg_start, pair_col, 70, 80, d_same, d_diff, *(() if kind == "sdtw" else (theta, gamma)))


# --------------------------------------------------------------------------- 7. the tools, end to end
N_UNITS = 20


def _make_corpus(root):
    """Twelve utterances of 80 .. 300 frames over 20 units in runs of 1 .. 5; two strings of 40 and 50 frames are planted twice each.
    Written as a unit file in the per-penalty layout of segment_quantization, and as one-hot .npy features."""
    rng = np.random.default_rng(77)
    lengths = [int(rng.integers(80, 301)) for _ in range(12)]
    lengths[2], lengths[7], lengths[4], lengths[10] = 200, 260, 180, 300
    utts = [U.draw_units(rng, m, N_UNITS) for m in lengths]
    planted = {}
    for (a, b), (oa, ob, size) in {(2, 7): (30, 150, 40), (4, 10): (100, 20, 50)}.items():
        # a string without a repeated neighbour, so that its alignment is one diagonal and its ends are sharp
        string = [int(rng.integers(0, N_UNITS))]
        while len(string) < size:
            string.append((string[-1] + int(rng.integers(1, N_UNITS))) % N_UNITS)
        string = np.asarray(string, dtype=np.int32)
        utts[a][oa:oa + size] = string
        utts[b][ob:ob + size] = string
        planted[(a, b)] = (oa, ob, size)
    names = [f"utt{k:02d}" for k in range(12)]
    penalty = root / "penalty_1.0"
    penalty.mkdir()
    (penalty / "quantized_outputs.txt").write_text("".join(f"/some/dir/{n}.flac\t" + ",".join(str(u) for u in v) + "\n"
                                                           for n, v in zip(names, utts)))
    feats = root / "features"
    feats.mkdir()
    for n, v in zip(names, utts):
        rows = np.zeros((len(v), N_UNITS), dtype=np.float32)
        rows[np.arange(len(v)), v] = 1
        np.save(feats / f"{n}.npy", rows)
    (root / "labels.txt").write_text("".join(f"{n} " + " ".join(str(u) for u in v) + "\n" for n, v in zip(names, utts)))
    return {"root": root, "units": penalty, "features": feats, "names": names, "utts": utts, "planted": planted}


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return _make_corpus(tmp_path_factory.mktemp("term_units"))


def _numbers(tree, skip=("args", "seconds")):
    """The numbers (and everything else) of a scores JSON, without the arguments and the timings."""
    return {k: v for k, v in tree.items() if k not in skip}


def test_detection_tool_from_units(corpus):
    root, names, planted = corpus["root"], corpus["names"], corpus["planted"]
    queries, relevance = [], []
    for k, ((a, b), (oa, ob, size)) in enumerate(planted.items()):
        # the query is the planted span of utterance a, which also stands in utterance b: on the feature grid an onset of
        # o / 100 + 0.002 and an offset of e / 100 + 0.008 cut frames o .. e - 1
        queries.append(f"q{k} {names[a]} {oa / 100 + 0.002:.3f} {(oa + size) / 100 + 0.008:.3f}\n")
        relevance.append(f"q{k} {names[b]} {ob / 100:.2f} {(ob + size) / 100:.2f}\n")
    queries.append(f"whole {names[0]}\n")
    relevance.append(f"whole {names[1]}\n")
    (root / "q.txt").write_text("".join(queries))
    (root / "r.txt").write_text("".join(relevance))
    common = ["--queries", str(root / "q.txt"), "--relevance", str(root / "r.txt"), "--distance_mode", "cosine", "--top", "5"]
    res_u = detection_tool.main(["from_units", str(corpus["units"]), "--out", str(root / "det_units"), *common])
    res_d = detection_tool.main(["from_pre_computed", str(corpus["features"]), "--file_extension", ".npy", "--out", str(root / "det_dense"),
                                 *common])
    assert res_u["score"].tobytes() == res_d["score"].tobytes() and np.array_equal(res_u["span"], res_d["span"])
    assert len(res_u["score"]) == 3 * 12 - 3                                     # a query is not scored against its own utterance
    text_u, text_d = (open(root / d / "detections.txt").read() for d in ("det_units", "det_dense"))
    assert text_u == text_d and len(text_u.splitlines()) == 15
    for k, ((a, b), (oa, ob, size)) in enumerate(planted.items()):               # the planted pair comes first, where it was put
        first = [ln.split() for ln in text_u.splitlines() if ln.startswith(f"q{k} ")][0]
        assert first == [f"q{k}", names[b], "1", "0", f"{ob / 100:.2f}", f"{(ob + size) / 100:.2f}", "1"], first
    scores_u, scores_d = (json.load(open(root / d / "term_detection_scores.json")) for d in ("det_units", "det_dense"))
    assert _numbers(scores_u) == _numbers(scores_d) and scores_u["map"] > 0.5 and scores_u["span_iou_at_0.5"] == 1.0
    log_u, log_d = (json.load(open(root / d / "term_detection_log.json")) for d in ("det_units", "det_dense"))
    assert (log_u["source"], log_u["distinct_units"], log_u["d_same"], log_u["d_diff"]) == ("from_units", N_UNITS, 0.0, 0.5)
    assert log_d["source"] == "from_pre_computed" and "d_same" not in log_d
    for key in ("documents", "queries", "pairs", "cells", "frames"):
        assert log_u[key] == log_d[key], key
    assert set(log_u["seconds"]) == set(detection_tool.STAGES)


def test_discovery_tool_from_units(corpus):
    root, names, planted = corpus["root"], corpus["names"], corpus["planted"]
    common = ["--distance_mode", "cosine", "--threshold", "0.25", "--gap_penalty", "0.125", "--pathPhone", str(root / "labels.txt")]
    res_u = discovery_tool.main(["from_units", str(corpus["units"] / "quantized_outputs.txt"), "--out", str(root / "disc_units"), *common])
    res_d = discovery_tool.main(["from_pre_computed", str(corpus["features"]), "--file_extension", ".npy", "--out", str(root / "disc_dense"),
                                 *common])
    assert res_u["score"].tobytes() == res_d["score"].tobytes() and np.array_equal(res_u["span"], res_d["span"])
    assert len(res_u["score"]) == 12 * 11 // 2
    for name in ("matches.txt", "classes.txt"):
        text_u, text_d = (open(root / d / name).read() for d in ("disc_units", "disc_dense"))
        assert text_u == text_d and text_u, name
    lines = [ln.split() for ln in open(root / "disc_units" / "matches.txt").read().splitlines()]
    found = {(ln[0], ln[3]): ln for ln in lines[:2]}                            # the planted pairs are the two best matches
    for (a, b), (oa, ob, size) in planted.items():
        ln = found[(names[a], names[b])]
        # the match holds the planted span on both sides (a chance agreement beside it may lengthen it, by a quarter at the most)
        for at, (first, last) in ((oa, (float(ln[1]), float(ln[2]))), (ob, (float(ln[4]), float(ln[5])))):
            assert first <= at / 100 + 1e-9 and last >= (at + size) / 100 - 1e-9 and last - first <= 1.25 * size / 100, ln
        assert float(ln[6]) >= 0.25 * size and int(ln[7]) >= size
    scores_u, scores_d = (json.load(open(root / d / "discovery_scores.json")) for d in ("disc_units", "disc_dense"))
    assert _numbers(scores_u) == _numbers(scores_d) and scores_u["n_matches"] == len(lines) >= 2
    log_u, log_d = (json.load(open(root / d / "discovery_log.json")) for d in ("disc_units", "disc_dense"))
    assert (log_u["source"], log_u["distinct_units"], log_u["d_same"], log_u["d_diff"]) == ("from_units", N_UNITS, 0.0, 0.5)
    assert log_u["distance_percentiles"] == {} and log_d["source"] == "from_pre_computed"
    for key in ("theta", "gamma", "utterances", "pairs", "cells", "frames", "pairs_with_a_match", "matches_selected", "matches_written"):
        assert log_u[key] == log_d[key], key
