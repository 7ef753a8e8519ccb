"""Spoken term discovery on the MI355X: cpc_local_align against the definition (tests/lalign_oracle.py), the work lists the planner
makes, and the command line end to end.

Exact family: frames whose distances and running gains are exact in f32 (one-hot rows under the cosine distance: d is 0 or 0.5,
theta 0.25, gamma 0.125; small integers in one column under the euclidian: theta 1.5, gamma 0.5).  Score bits and all five span
integers EQUAL the f32 statement on every pair, ties included.  Row lengths (1, 2, 63, 64, 65, 128, 129, 193) against column
lengths (1, 2, 63, 64, 65, 127, 130, 257): the smallest shapes that cross the strip seams at 64 / 128 / 192 rows and the tile seams
at 64 / 128 / 256 columns.

Real-valued family: Gaussian frames, theta a little below the typical distance and a small gamma, so that the best paths are long
and take horizontal and vertical steps (measured: up to 233 / 404 cells with 737 / 1 924 such steps over the 72 pairs).  Integers
and score are compared on CLEAR pairs (lalign_oracle), the score within 1e-5 RELATIVE of the float64 statement, and at most 10 %
of the pairs may be unclear.  Measured with the committed statement alone, on the CPU: 1 of 72 pairs unclear with the cosine
distance, 0 of 72 with the euclidian, 0 of 4 at D = 256 with either; 0 of 40 in the planted family."""
import json
from fractions import Fraction

import numpy as np
import pytest
import torch

from cpc2_amd import _lib
from cpc2_amd import term_detection as td
from cpc2_amd import term_discovery as tdisc
from cpc2_amd.eval import term_discovery as tool
from cpc2_amd.eval.ABX import abx_iterators as abx_it
from tests import lalign_oracle as L

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CAP = 8192                                                    # workgroups per launch
EXACT_N = (1, 2, 63, 64, 65, 128, 129, 193)                   # up to four strips
EXACT_M = (1, 2, 63, 64, 65, 127, 130, 257)
EXACT_PARAMS = {"cosine": (0.25, 0.125), "euclidian": (1.5, 0.5)}
REAL_N = (1, 2, 5, 31, 63, 64, 65, 100, 129)
REAL_M = (1, 7, 63, 64, 65, 130, 200, 300)
REAL_PARAMS = {("cosine", 36): (0.47, 0.02), ("euclidian", 36): (7.8, 0.3), ("cosine", 256): (0.49, 0.01), ("euclidian", 256): (22.0, 0.3)}


# --------------------------------------------------------------------------- inputs
def _pack(items, dp, gap=0):
    """Items as one [total, dp] buffer (padding columns zero) with `gap` NaN rows before, between and behind them."""
    rows, offs, lens, at = [], [], [], 0
    for v in items:
        if gap:
            rows.append(np.full((gap, dp), np.nan, dtype=np.float32))
            at += gap
        block = np.zeros((v.shape[0], dp), dtype=np.float32)
        block[:, :v.shape[1]] = v
        rows.append(block)
        offs.append(at)
        lens.append(v.shape[0])
        at += v.shape[0]
    if gap:
        rows.append(np.full((gap, dp), np.nan, dtype=np.float32))
    frames = torch.from_numpy(np.concatenate(rows)).to(DEV)
    return frames, torch.tensor(offs, dtype=torch.int32, device=DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), lens


def _run_plan(frames, off, lens, plan, lens_host, distance, theta, gamma, scratch_fill=None):
    seg_a, seg_start, pair_b = plan[:3]
    max_a, max_b = int(np.asarray(lens_host)[seg_a].max()), int(np.asarray(lens_host)[pair_b].max())
    scratch = None
    if scratch_fill is not None:
        nbytes = _lib.load().cpc_local_align_scratch_bytes(len(seg_a), max_a, max_b)
        scratch = torch.full((max(nbytes, 1),), scratch_fill, dtype=torch.uint8, device=DEV)
    score, span = tdisc.run_segments(frames, off, lens, torch.from_numpy(seg_a).to(DEV), torch.from_numpy(seg_start).to(DEV),
                                     torch.from_numpy(pair_b).to(DEV), max_a, max_b, td.distance_code(distance), theta, gamma,
                                     scratch=scratch)
    return score.cpu().numpy(), span.cpu().numpy()


def _all_pairs(rows, cols, distance, dp, theta, gamma, gap=0, cell_budget=None, scratch_fill=None):
    """Every row item against every column item: score [R, C] f32 and span [R, C, 5], on the host."""
    frames, off, lens, lens_host = _pack(list(cols) + list(rows), dp, gap)
    nc = len(cols)
    plan = td.plan_segments(np.arange(nc, nc + len(rows)), np.arange(nc), lens_host, cell_budget=cell_budget)
    assert np.array_equal(plan[3], np.repeat(np.arange(len(rows)), nc)) and np.array_equal(plan[2], np.tile(np.arange(nc), len(rows)))
    score, span = _run_plan(frames, off, lens, plan, lens_host, distance, theta, gamma, scratch_fill)
    return score.reshape(len(rows), nc), span.reshape(len(rows), nc, 5)


def _exact_items(rng, n, distance):
    v = np.zeros((n, 4), dtype=np.float32)
    if distance == "euclidian":                               # |a - b| of small integers in column 0: dp = 4
        v[:, 0] = rng.integers(-3, 4, n)
    else:                                                     # one-hot rows: the distance is 0 or acos(0) / pi = 0.5
        v[np.arange(n), rng.integers(0, 4, n)] = 1.0
    return v


def _real_items(rng, n, distance, width=36):
    if distance == "cosine":                                  # width - 1 drawn columns + the singularity column
        v = torch.from_numpy(rng.standard_normal((n, width - 1)).astype(np.float32))
        return abx_it.normalize_with_singularity(v).numpy()
    return rng.standard_normal((n, width - 3)).astype(np.float32)    # three columns of padding


# --------------------------------------------------------------------------- exact family
@pytest.fixture(scope="module", params=["euclidian", "cosine"])
def exact(request):
    distance = request.param
    theta, gamma = EXACT_PARAMS[distance]
    rng = np.random.default_rng(17 if distance == "cosine" else 16)
    rows = [_exact_items(rng, n, distance) for n in EXACT_N]
    cols = [_exact_items(rng, m, distance) for m in EXACT_M]
    want = [[L.local_align_f32(L.frame_distances(a, b, distance), theta, gamma) for b in cols] for a in rows]
    return distance, rows, cols, want, theta, gamma


def _assert_exact(score, span, want):
    for i, row in enumerate(want):
        for j, (v, cells) in enumerate(row):
            assert type(v) is np.float32
            assert score[i, j].tobytes() == v.tobytes(), (i, j, score[i, j], v)
            assert tuple(span[i, j]) == cells, (i, j, span[i, j], cells)


def test_exact_family_equals_the_f32_statement(exact):
    distance, rows, cols, want, theta, gamma = exact
    score, span = _all_pairs(rows, cols, distance, 4, theta, gamma)
    assert sum(v > 0 for row in want for v, _c in row) >= 60 and any(c[4] > 64 for row in want for _v, c in row)
    _assert_exact(score, span, want)


def test_split_lists_gaps_scratch_and_repeat_give_the_same_bits(exact):
    """One segment per pair, one segment per row item and the default plan; items packed with NaN rows between them; a scratch
    that holds NaN (0xFFFFFFFF) or zeros before the launch; the same launch twice."""
    distance, rows, cols, want, theta, gamma = exact
    base = _all_pairs(rows, cols, distance, 4, theta, gamma)
    for kwargs in ({"cell_budget": 1}, {"cell_budget": 10 ** 12}, {"cell_budget": 20_000}, {"gap": 3}, {"scratch_fill": 0xFF},
                   {"scratch_fill": 0x00}, {}):
        other = _all_pairs(rows, cols, distance, 4, theta, gamma, **kwargs)
        assert base[0].tobytes() == other[0].tobytes() and np.array_equal(base[1], other[1]), kwargs
    _assert_exact(*_all_pairs(rows, cols, distance, 4, theta, gamma, gap=5, cell_budget=10 ** 12, scratch_fill=0xFF), want)


# --------------------------------------------------------------------------- work lists
@pytest.mark.parametrize("n", [3, 65])
def test_more_segments_than_the_grid_cap(n):
    """2 * 8192 + 3 segments of one pair each, items of 1 .. 3 frames: every workgroup takes a second and a third segment.  With
    row items of 65 frames (two strips) it also reuses its boundary rows from segment to segment; they hold NaN before the launch."""
    rng = np.random.default_rng(31)
    cols = [_exact_items(rng, 1 + k % 3, "euclidian") for k in range(11)]
    rows = [_exact_items(rng, n if n > 3 else 1 + k % 3, "euclidian") for k in range(7)]
    frames, off, lens, lens_host = _pack(cols + rows, 4)
    n_seg = 2 * CAP + 3
    seg_a = (11 + np.arange(n_seg) % 7).astype(np.int32)
    pair_b = ((np.arange(n_seg) * 5) % 11).astype(np.int32)
    assert _lib.load().cpc_local_align_scratch_bytes(n_seg, n, 3) == (CAP * 2 * 12 * 3 if n > 64 else 0)
    score, span = _run_plan(frames, off, lens, (seg_a, np.arange(n_seg + 1, dtype=np.int32), pair_b), lens_host, "euclidian", 1.5, 0.5,
                            scratch_fill=0xFF)
    want = {(a, b): L.local_align_f32(L.frame_distances(rows[a], cols[b], "euclidian"), 1.5, 0.5) for a in range(7) for b in range(11)}
    want_score = np.array([want[(a - 11, b)][0] for a, b in zip(seg_a, pair_b)], dtype=np.float32)
    want_span = np.array([want[(a - 11, b)][1] for a, b in zip(seg_a, pair_b)], dtype=np.int32)
    assert score.tobytes() == want_score.tobytes() and np.array_equal(span, want_span)


def test_pairs_of_a_segment_share_the_boundary_rows():
    """Row items of two and three strips against several column items in one segment, a long pair followed by a short one: a
    workgroup's boundary rows and its lanes' registers serve one pair after the other, and nothing of the first leaks into the
    second.  The first row item ends in a strong match against the long column item; the short column item matches nothing."""
    rng = np.random.default_rng(37)
    cols = [_exact_items(rng, m, "euclidian") for m in (130, 5, 70)]
    rows = [_exact_items(rng, n, "euclidian") for n in (129, 65, 3)]
    rows[0][-40:, 0] = cols[0][-40:, 0]                        # a long match that ends in the last cell of the long pair
    cols[1][:, 0] = 50.0                                       # far from everything: no positive cell
    frames, off, lens, lens_host = _pack(cols + rows, 4)
    seg_a = np.array([3, 4, 5, 4, 3], dtype=np.int32)
    seg_start = np.array([0, 3, 5, 8, 9, 12], dtype=np.int32)
    pair_b = np.array([0, 1, 2, 2, 1, 0, 1, 2, 0, 2, 0, 1], dtype=np.int32)
    assert _lib.load().cpc_local_align_scratch_bytes(5, 129, 130) == 5 * 2 * 12 * 130
    outs = [_run_plan(frames, off, lens, (seg_a, seg_start, pair_b), lens_host, "euclidian", 1.5, 0.5, scratch_fill=fill)
            for fill in (0x00, 0xFF)]
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and np.array_equal(outs[0][1], outs[1][1])
    seg_of_pair = np.repeat(np.arange(5), np.diff(seg_start))
    for p, b in enumerate(pair_b.tolist()):
        a = int(seg_a[seg_of_pair[p]]) - 3
        v, cells = L.local_align_f32(L.frame_distances(rows[a], cols[b], "euclidian"), 1.5, 0.5)
        assert outs[0][0][p].tobytes() == v.tobytes() and tuple(outs[0][1][p]) == cells, p
    assert outs[0][0][0] >= 40 * 1.5 and tuple(outs[0][1][0][[1, 3]]) == (128, 129)
    assert outs[0][0][1] == 0.0 and (outs[0][1][1] == -1).all()             # the short pair behind the long one: nothing leaked


# --------------------------------------------------------------------------- real-valued family
def _assert_clear_pairs(score, span, table, cap=0.10):
    unclear = 0
    for i, row in enumerate(table):
        for j, (v, cells, clear) in enumerate(row):
            print(f"pair {i} {j}: kernel {score[i, j]!r} {tuple(span[i, j])} definition {v!r} {cells} clear {clear}")
            if not clear:
                unclear += 1
                continue
            assert tuple(span[i, j]) == cells, (i, j, span[i, j], cells)
            assert abs(float(score[i, j]) - v) <= 1e-5 * abs(v), (i, j, score[i, j], v)
    n = sum(len(row) for row in table)
    assert unclear <= cap * n, (unclear, n)


@pytest.mark.parametrize("distance", ["cosine", "euclidian"])
def test_real_valued_family_on_clear_pairs(distance):
    theta, gamma = REAL_PARAMS[(distance, 36)]
    rng = np.random.default_rng(0)
    rows = [_real_items(rng, n, distance) for n in REAL_N]
    cols = [_real_items(rng, m, distance) for m in REAL_M]
    table = [[L.local_align(L.frame_distances(a, b, distance), np.float32(theta), np.float32(gamma)) for b in cols] for a in rows]
    score, span = _all_pairs(rows, cols, distance, 36, theta, gamma)
    _assert_clear_pairs(score, span, table)


@pytest.mark.parametrize("distance", ["cosine", "euclidian"])
def test_real_valued_family_at_256_features(distance):
    """D = 256: eight chunks of the staged feature columns per tile."""
    theta, gamma = REAL_PARAMS[(distance, 256)]
    rng = np.random.default_rng(0)
    rows = [_real_items(rng, n, distance, 256) for n in (65, 129)]
    cols = [_real_items(rng, m, distance, 256) for m in (64, 130)]
    table = [[L.local_align(L.frame_distances(a, b, distance), np.float32(theta), np.float32(gamma)) for b in cols] for a in rows]
    score, span = _all_pairs(rows, cols, distance, 256, theta, gamma)
    _assert_clear_pairs(score, span, table, cap=0.0)


@pytest.mark.parametrize("distance", ["cosine", "euclidian"])
def test_planted_fragments_are_found_on_the_device(distance):
    """The planted family through local_alignment: every shared fragment is found within 4 frames.  In euclidian mode the kernel
    also agrees with the definition on clear pairs; in cosine mode the matched frames' dot products sit near 1, where f32 acos is
    the limit tests/test_abx_cpu.py documents, so only the spans are held to the planted ones there."""
    cases = []
    for n, m, draw in L.PLANTED:
        rng = np.random.default_rng(1000 * n + m + draw)
        a, b, want = L.planted_pair(rng, n, m)
        if distance == "cosine":
            a, b = L.unit_rows(a), L.unit_rows(b)
        cases.append((a.astype(np.float32), b.astype(np.float32), want))
    k = len(cases)
    items = [c[0] for c in cases] + [c[1] for c in cases]
    frames, off, lens, lens_host = _pack(items, 16)
    thetas = [np.float32(L.planted_theta(L.frame_distances(c[0], c[1], distance), distance)) for c in cases]
    table = []
    for i, (a, b, want) in enumerate(cases):                   # theta differs from pair to pair in euclidian mode: one call each
        theta = float(thetas[i])
        score, span, pair_a, pair_b = tdisc.local_alignment(frames, off, lens, [i, k + i], distance, theta, theta / 2, lens_host=lens_host)
        assert pair_a.tolist() == [i] and pair_b.tolist() == [k + i]
        score, span = score.cpu().numpy(), span.cpu().numpy()
        assert score[0] > 0 and max(abs(int(span[0, c]) - want[c]) for c in range(4)) <= 4, (L.PLANTED[i], span[0], want)
        if distance == "euclidian":
            row = [L.local_align(L.frame_distances(a, b, distance), np.float32(theta), np.float32(theta / 2))]
            _assert_clear_pairs(score.reshape(1, 1), span.reshape(1, 1, 5), [row], cap=1.0)
            table.append(row[0][2])
    assert distance == "cosine" or sum(1 for c in table if not c) <= 0.10 * k


# --------------------------------------------------------------------------- not computable, bad arguments
def test_uncomputable_pairs_and_bad_arguments():
    rng = np.random.default_rng(41)
    items = [_exact_items(rng, n, "euclidian") for n in (5, 70, 9, 80)]
    frames, off, lens, _ = _pack(items, 4)
    lens_zero = torch.cat([lens, torch.zeros(1, dtype=torch.int32, device=DEV)])       # item 4: no frame
    off_zero = torch.cat([off, torch.zeros(1, dtype=torch.int32, device=DEV)])
    # segments: row item 0 (5 frames), 1 (70 frames), 7 (out of range), 4 (empty), 3 (80 frames: longer than max_len_a = 70)
    seg_a = torch.tensor([0, 1, 7, 4, 3], dtype=torch.int32, device=DEV)
    seg_start = torch.tensor([0, 4, 9, 10, 11, 12], dtype=torch.int32, device=DEV)
    pair_b = torch.tensor([2, -1, 3, 4, 2, 5, 1, 0, 3, 0, 0, 0], dtype=torch.int32, device=DEV)
    lib = _lib.load()

    def check_edges(max_b=80):
        score, span = tdisc.run_segments(frames, off_zero, lens_zero, seg_a, seg_start, pair_b, 70, max_b, td.EUCLIDIAN, 1.5, 0.5)
        score, span = score.cpu().numpy(), span.cpu().numpy()
        nan = [1, 3, 5, 9, 10, 11]                              # index -1, empty column item, index 5, row out of range, empty row,
        ok = {0: (0, 2), 2: (0, 3), 4: (1, 2), 6: (1, 1), 7: (1, 0), 8: (1, 3)}      # row longer than max_len_a
        if max_b < 80:                                         # a column item longer than max_len_b
            nan += [2, 8]
            del ok[2], ok[8]
        assert np.isnan(score[nan]).all() and (span[nan] == -1).all()
        for p, (a, b) in ok.items():
            v, cells = L.local_align_f32(L.frame_distances(items[a], items[b], "euclidian"), 1.5, 0.5)
            assert score[p].tobytes() == v.tobytes() and tuple(span[p]) == cells, p
        assert score[6] >= 70 * 1.5 and span[6, 4] >= 70       # an item against itself: its diagonal is one of the paths

    check_edges()
    check_edges(max_b=79)
    one = torch.zeros(16, dtype=torch.int32, device=DEV)
    rows = torch.zeros(16, dtype=torch.float32, device=DEV)
    out_score = torch.full((4,), 77.0, dtype=torch.float32, device=DEV)
    out_span = torch.full((4, 5), 77, dtype=torch.int32, device=DEV)
    small = torch.zeros(64, dtype=torch.uint8, device=DEV)

    def call(frames=rows, dp=4, n_items=1, n_seg=1, max_la=4, max_lb=4, distance=td.COSINE, theta=0.25, gamma=0.125, score=out_score,
             span=out_span, seg_a=one, scratch=None, scratch_bytes=0):
        return lib.cpc_local_align(_lib.ptr(frames), dp, _lib.ptr(one), _lib.ptr(one), n_items, _lib.ptr(seg_a), _lib.ptr(one),
                                   _lib.ptr(one), n_seg, max_la, max_lb, distance, theta, gamma, _lib.ptr(score), _lib.ptr(span),
                                   _lib.ptr(scratch), scratch_bytes, _lib.stream_ptr(DEV))

    inf, nan = float("inf"), float("nan")
    for kwargs, word, status in (({"dp": 6}, "multiple of 4", -1), ({"dp": 0}, "multiple of 4", -1), ({"dp": -4}, "multiple of 4", -1),
                                 ({"distance": 2}, "unknown distance", -1), ({"distance": -1}, "unknown distance", -1),
                                 ({"frames": None}, "null buffer", -1), ({"score": None}, "null buffer", -1),
                                 ({"span": None}, "null buffer", -1), ({"seg_a": None}, "null buffer", -1),
                                 ({"n_items": 0}, "bad sizes", -1), ({"n_seg": -1}, "bad sizes", -1), ({"max_lb": 0}, "bad sizes", -1),
                                 ({"max_la": 0}, "bad sizes", -1), ({"max_la": -3}, "bad sizes", -1),
                                 ({"max_la": 32768}, "at most 32767", -1), ({"max_lb": 32768}, "at most 32767", -1),
                                 ({"theta": 0.0}, "theta", -1), ({"theta": -0.25}, "theta", -1), ({"theta": nan}, "theta", -1),
                                 ({"theta": inf}, "theta", -1), ({"gamma": -0.125}, "gamma", -1), ({"gamma": nan}, "gamma", -1),
                                 ({"gamma": inf}, "gamma", -1), ({"max_la": 65}, "scratch", -3),
                                 ({"max_la": 65, "scratch": small, "scratch_bytes": 64}, "scratch", -3)):
        got = call(**kwargs)
        assert got == status, (kwargs, got)                      # CPC_ERR_INVALID / CPC_ERR_WORKSPACE
        assert word in lib.cpc_last_error().decode(), (kwargs, lib.cpc_last_error())
        with pytest.raises(ValueError if status == -1 else RuntimeError, match=word):
            _lib.check(got, "cpc_local_align")
    assert call(n_seg=0) == 0                                    # nothing to do: OK, and nothing written
    assert call(gamma=0.0, n_seg=0) == 0                         # gamma = 0 is allowed
    torch.cuda.synchronize()
    assert (out_score == 77.0).all() and (out_span == 77).all()  # every refusal left the outputs untouched
    check_edges()                                                # a refusal leaves the next valid call intact
    assert lib.cpc_local_align_scratch_bytes(20000, 65, 500) == lib.cpc_local_align_scratch_bytes(CAP, 65, 500) == CAP * 2 * 12 * 500
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tdisc.run_segments(frames.cpu(), off, lens, seg_a, seg_start, pair_b, 70, 80, td.EUCLIDIAN, 1.5, 0.5)


# --------------------------------------------------------------------------- end to end
def _levenshtein(a, b):
    row = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        new = [i]
        for j, y in enumerate(b, 1):
            new.append(min(row[j] + 1, new[j - 1] + 1, row[j - 1] + (x != y)))
        row = new
    return row[-1]


@pytest.mark.parametrize("distance", ["euclidian", "cosine"])
def test_end_to_end_on_pre_computed_features(tmp_path, distance):
    """Five .npy utterances of prototypes of their own; three pairs of them share a planted fragment (40 frames, 15 % dropped and
    0.05 noise on one side), and frame labels are given.  matches.txt names the planted pairs first, line by line as the definition
    has them, and discovery_scores.json equals the exact-fraction statement on the definition's matches."""
    rng = np.random.default_rng(202)
    lengths = (150, 210, 180, 260, 140)
    utts = [L.speech_like(rng, m) for m in lengths]
    labels = []
    for m in lengths:
        row = []
        while len(row) < m:
            row += [int(rng.integers(0, 9))] * int(rng.integers(2, 9))
        labels.append(row[:m])
    planted = {}
    for (a, b), (oa, ob) in {(0, 1): (20, 150), (2, 3): (100, 30), (1, 4): (60, 80)}.items():
        frag = L.speech_like(rng, 40)
        keep = np.sort(rng.choice(40, 34, replace=False))
        utts[a][oa:oa + 40] = frag
        utts[b][ob:ob + 34] = frag[keep] + 0.05 * rng.standard_normal((34, 16))
        frag_labels = np.repeat(rng.integers(0, 9, 8), 5)
        labels[a][oa:oa + 40] = frag_labels.tolist()
        labels[b][ob:ob + 34] = frag_labels[keep].tolist()
        planted[(a, b)] = (oa + int(keep[0]), oa + int(keep[-1]), ob, ob + 33)
    utts = [u.astype(np.float32) for u in utts]
    feat_dir = tmp_path / "features"
    feat_dir.mkdir()
    for i, u in enumerate(utts):
        np.save(feat_dir / f"utt{i}.npy", u)
    (tmp_path / "labels.txt").write_text("".join(f"utt{i} " + " ".join(str(x) for x in row) + "\n" for i, row in enumerate(labels)))
    theta_arg = "0.25" if distance == "cosine" else "2.8"
    out = tmp_path / "out"
    res = tool.main(["from_pre_computed", str(feat_dir), "--file_extension", ".npy", "--threshold", theta_arg, "--out", str(out),
                     "--distance_mode", distance, "--pathPhone", str(tmp_path / "labels.txt")])
    log = json.load(open(out / "discovery_log.json"))
    scores = json.load(open(out / "discovery_scores.json"))
    theta = float(np.float32(float(theta_arg)))
    gamma = float(np.float32(theta / 2))
    assert log["theta"] == theta and log["gamma"] == gamma and log["utterances"] == 5 and log["pairs"] == 10
    assert set(log["distance_percentiles"]) == {"1", "5", "10", "25", "50"} and set(log["seconds"]) == set(tool.STAGES)
    assert log["cells"] == sum(lengths[a] * lengths[b] for a in range(5) for b in range(a + 1, 5))
    assert log["empty"] == log["too_long"] == log["non_finite"] == []

    # the definition on the rows the tool searched
    rows = [abx_it.normalize_with_singularity(torch.from_numpy(u.copy())).numpy() for u in utts] if distance == "cosine" else utts
    if distance == "cosine":
        # no frame is within 1 - 1e-4 of a frame of another utterance: acos has a slope below 1 / sqrt(2e-4) = 71 there, and an f32
        # dot product's few ulps of 1 move a distance by less than 6e-6 (the bound of tests/test_term_detection_gpu.py)
        assert max(float((rows[a].astype(np.float64) @ rows[b].astype(np.float64).T).max()) for a in range(5) for b in range(a + 1, 5)) < 1 - 1e-4
    table = {(a, b): L.local_align(L.frame_distances(rows[a], rows[b], distance), theta, gamma) for a in range(5) for b in range(a + 1, 5)}
    pairs = sorted(table)
    kept = [p for p in pairs if table[p][0] > 0 and min(table[p][1][1] - table[p][1][0], table[p][1][3] - table[p][1][2]) + 1 >= 25]
    kept.sort(key=lambda p: (-table[p][0], pairs.index(p)))
    assert set(kept[:3]) == set(planted)                                        # the planted pairs come first
    assert all(table[p][2] for p in kept), [table[p] for p in kept]              # and the kept pairs are clear
    for p, want in planted.items():
        assert max(abs(table[p][1][c] - want[c]) for c in range(4)) <= 4, (p, table[p], want)
    # no pair sits at the selection's edge: the kernel's error (1e-5 relative) cannot move one in or out, or swap two
    vs = [table[p][0] for p in kept]
    assert all(a - b > 1e-4 * a for a, b in zip(vs, vs[1:]))
    lines = [ln.split() for ln in open(out / "matches.txt").read().splitlines()]
    assert len(lines) == len(kept) == log["matches_written"]
    for ln, p in zip(lines, kept):
        v, (si, ei, sj, ej, length), _clear = table[p]
        assert ln[0] == f"utt{p[0]}" and ln[3] == f"utt{p[1]}"
        assert (ln[1], ln[2], ln[4], ln[5]) == (f"{si / 100:.2f}", f"{(ei + 1) / 100:.2f}", f"{sj / 100:.2f}", f"{(ej + 1) / 100:.2f}")
        assert abs(float(ln[6]) - v) <= 2e-5 * v and int(ln[7]) == length       # 1e-5 of the kernel + the 8 digits written
    classes = open(out / "classes.txt").read().split("\n\n")
    assert classes[0].splitlines() == ["Class 0", " ".join([lines[0][0], lines[0][1], lines[0][2]]), " ".join(lines[0][3:6])]
    assert len([c for c in classes if c.strip()]) == len(kept)

    # NED and coverage as fractions, from the definition's matches
    parts, covered = [], set()
    for p in kept:
        si, ei, sj, ej, _length = table[p][1]
        sa, sb = tdisc.fragment_phones(labels[p[0]], si, ei), tdisc.fragment_phones(labels[p[1]], sj, ej)
        assert sa and sb
        parts.append(Fraction(_levenshtein(sa, sb), max(len(sa), len(sb))))
        covered |= {(p[0], t) for t in range(si, ei + 1)} | {(p[1], t) for t in range(sj, ej + 1)}
    want_ned = sum(parts) / len(parts)
    assert abs(Fraction(scores["ned"]) - want_ned) <= 4 * Fraction(2.0 ** -53) * max(want_ned, Fraction(1, 10 ** 9))
    assert (scores["covered_frames"], scores["total_frames"]) == (len(covered), sum(lengths))
    assert scores["coverage"] == len(covered) / sum(lengths)
    assert scores["n_matches"] == scores["n_ned_pairs"] == len(kept) and scores["n_empty_pairs"] == scores["n_unlabelled_pairs"] == 0
    assert scores["n_files_with_fragment"] == 5 and scores["theta"] == theta
    assert res["scores"]["ned"] == scores["ned"] and [tuple(m[:1] + m[3:4]) for m in res["matches"]] == [(f"utt{a}", f"utt{b}") for a, b in kept]
    # a second run into the same directory is refused: nothing is overwritten
    with pytest.raises(ValueError, match="--out"):
        tool.main(["from_pre_computed", str(feat_dir), "--file_extension", ".npy", "--threshold", theta_arg, "--out", str(out)])
