"""Spoken term discovery without a GPU: the restatement of the local alignment (tests/lalign_oracle.py) on hand-made matrices and
on the planted family, the pair planner, the host side of the scores, the command line's refusals and the ABI."""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from cpc2_amd import _lib
from cpc2_amd import term_discovery as tdisc
from cpc2_amd.eval import term_discovery as tool
from tests import lalign_oracle as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT_N = (1, 2, 63, 64, 65, 128, 129, 193)
EXACT_M = (1, 2, 63, 64, 65, 127, 130, 257)


# --------------------------------------------------------------------------- the restatement itself
def test_hand_made_matrices_pin_the_rules():
    theta, gamma = 0.25, 0.125
    # no positive cell: every distance is at or above the threshold (a gain of exactly 0 does not open a cell)
    assert L.local_align_f32(np.full((3, 4), 0.5), theta, gamma) == (np.float32(0), L.NONE)
    assert L.local_align_f32(np.full((3, 4), 0.25), theta, gamma) == (np.float32(0), L.NONE)
    assert L.local_align(np.full((3, 4), 0.5), theta, gamma) == (0.0, L.NONE, True)
    # one frame each
    assert L.local_align_f32([[0.0]], theta, gamma) == (np.float32(0.25), (0, 0, 0, 0, 1))
    assert L.local_align_f32([[0.5]], theta, gamma) == (np.float32(0), L.NONE)
    # an exact diagonal of three zeros inside 0.5: rows 1..3 against columns 2..4
    d = np.full((5, 6), 0.5)
    for k in range(3):
        d[1 + k, 2 + k] = 0.0
    assert L.local_align_f32(d, theta, gamma) == (np.float32(0.75), (1, 3, 2, 4, 3))
    assert L.local_align(d, theta, gamma) == (0.75, (1, 3, 2, 4, 3), True)
    # a NaN distance closes its cell: the diagonal is cut in two, the first half wins the tie (smallest i)
    d = np.full((4, 4), 0.5)
    d[np.arange(4), np.arange(4)] = 0.0
    d[2, 2] = np.nan
    assert L.local_align_f32(d, theta, gamma) == (np.float32(0.5), (0, 1, 0, 1, 2))
    # a tie between diag and left.  H[0][1] = 0.25 opens at (0, 1); H[1][0] = 0.25 opens at (1, 0); H[1][1] = 0.25 + 0.125 follows
    # left (left and up tie at 0.125: left wins), start (1, 0), length 2.  Cell (1, 2): diag = H[0][1] = 0.25, left = 0.375 - 0.125
    # = 0.25.  diag wins: start (0, 1), length 2, not start (1, 0), length 3.
    d = np.array([[0.5, 0.0, 0.5],
                  [0.0, 0.0, 0.0]])
    score, span = L.local_align_f32(d, theta, gamma)
    assert (score, span) == (np.float32(0.5), (0, 1, 1, 2, 2))
    assert L.local_align(d, theta, gamma) == (0.5, (0, 1, 1, 2, 2), False)                # the tie makes the pair unclear
    # the same matrix with the diag candidate lowered to 0.125: left wins and carries the longer path
    d[0, 1] = 0.125
    assert L.local_align_f32(d, theta, gamma) == (np.float32(0.5), (1, 1, 0, 2, 3))
    # a tie between left and up at (1, 1): left = H[1][0] - gamma, up = H[0][1] - gamma, both 0.125; left wins (start (1, 0))
    d = np.array([[0.5, 0.0],
                  [0.0, 0.0]])
    assert L.local_align_f32(d, theta, gamma) == (np.float32(0.375), (1, 1, 0, 1, 2))
    # two equal maxima: the smallest i, then the smallest j
    d = np.full((3, 5), 0.5)
    d[2, 0] = d[0, 3] = d[0, 1] = 0.0
    assert L.local_align_f32(d, theta, gamma) == (np.float32(0.25), (0, 0, 1, 1, 1))
    d[0, 1] = 0.5
    assert L.local_align_f32(d, theta, gamma) == (np.float32(0.25), (0, 0, 3, 3, 1))
    d[0, 3] = 0.5
    assert L.local_align_f32(d, theta, gamma) == (np.float32(0.25), (2, 2, 0, 0, 1))
    # gamma = 0: a closed neighbour's 0 is not worth continuing (best <= 0 opens)
    assert L.local_align_f32([[0.5, 0.0]], theta, 0.0) == (np.float32(0.25), (0, 0, 1, 1, 1))
    # unclear: a second cell within the margin of the best
    d = np.full((3, 3), 0.5)
    d[0, 0], d[2, 2] = 0.0, 1e-7
    assert L.local_align(d, theta, gamma)[2] is False
    d[2, 2] = 0.01
    assert L.local_align(d, theta, gamma) == (0.25, (0, 0, 0, 0, 1), True)
    # unclear: a clamp decision within the margin of 0 while nothing else is positive
    assert L.local_align([[0.25 - 1e-7]], theta, gamma)[2] is False


def _exact_items(rng, n, distance):
    v = np.zeros((n, 4), dtype=np.float32)
    if distance == "euclidian":
        v[:, 0] = rng.integers(-3, 4, n)
    else:
        v[np.arange(n), rng.integers(0, 4, n)] = 1.0
    return v


@pytest.mark.parametrize("distance,theta,gamma", [("cosine", 0.25, 0.125), ("euclidian", 1.5, 0.5)])
def test_f32_statement_equals_the_f64_statement_on_the_exact_family(distance, theta, gamma):
    """The exact family of the GPU test: one-hot rows under the cosine distance (d is 0 or 0.5) and small integers in one column
    under the euclidian, row lengths EXACT_N against column lengths EXACT_M.  Every sum is exact in f32, so the two programs agree
    to the bit, ties included."""
    rng = np.random.default_rng(17 if distance == "cosine" else 16)
    rows = [_exact_items(rng, n, distance) for n in EXACT_N]
    cols = [_exact_items(rng, m, distance) for m in EXACT_M]
    for a in rows:
        for b in cols:
            d = L.frame_distances(a, b, distance)
            s32, span32 = L.local_align_f32(d, theta, gamma)
            s64, span64, _clear = L.local_align(d, theta, gamma)
            assert float(s32) == s64 and span32 == span64, (len(a), len(b))


def test_planted_family_is_found_and_clear():
    """Two unrelated speech-like items that share a fragment of 30 frames, 15 % of them dropped and 0.05 noise on one side; theta
    0.25 (cosine) or half the median distance (euclidian), gamma = theta / 2.  Measured with this module's statement: 40 of 40
    spans within 4 frames of the planted one (the largest deviation is 3 frames: a dropped first frame that the other side's
    run still matches), 0 of 40 pairs unclear."""
    found = unclear = 0
    for distance in ("cosine", "euclidian"):
        for n, m, draw in L.PLANTED:
            rng = np.random.default_rng(1000 * n + m + draw)
            a, b, want = L.planted_pair(rng, n, m)
            if distance == "cosine":
                a, b = L.unit_rows(a), L.unit_rows(b)
            d = L.frame_distances(a, b, distance)
            theta = L.planted_theta(d, distance)
            score, span, clear = L.local_align(d, theta, theta / 2)
            print(distance, n, m, draw, score, span, want, clear)
            assert score > 0
            assert max(abs(span[k] - want[k]) for k in range(4)) <= 4, (distance, n, m, draw, span, want)
            found += 1
            unclear += not clear
    assert found == 40 and unclear <= 0.10 * 40, (found, unclear)


# --------------------------------------------------------------------------- planner
def test_plan_pairs_lists_every_unordered_pair_once():
    rng = np.random.default_rng(3)
    lens = rng.integers(1, 400, 23)
    items = np.arange(23)
    exclude = [(2, 5), (9, 4), (0, 22), (7, 7)]
    dropped = {(2, 5), (4, 9), (0, 22)}
    plans = {}
    for budget in (1, 20_000, 10 ** 12, None):
        seg_a, seg_start, pair_b, pair_a = tdisc.plan_pairs(items, lens, exclude=exclude, cell_budget=budget)
        pairs = list(zip(pair_a.tolist(), pair_b.tolist()))
        assert all(a < b for a, b in pairs)
        assert len(set(pairs)) == len(pairs) == 23 * 22 // 2 - 3
        assert set(pairs) == {(a, b) for a in range(23) for b in range(a + 1, 23)} - dropped
        assert seg_start[0] == 0 and seg_start[-1] == len(pairs) and (np.diff(seg_start) >= 1).all()
        for s, a in enumerate(seg_a):                               # a segment holds pairs of its row item only
            assert (pair_a[seg_start[s]:seg_start[s + 1]] == a).all()
            cells = int(lens[a]) * int(lens[pair_b[seg_start[s]:seg_start[s + 1]]].sum())
            if budget is not None and seg_start[s + 1] - seg_start[s] > 1:
                assert cells <= budget
        plans[budget] = pairs
        assert seg_a.dtype == seg_start.dtype == pair_b.dtype == pair_a.dtype == np.int32
    assert plans[1] == plans[20_000] == plans[10 ** 12] == plans[None]
    assert len(tdisc.plan_pairs(items, lens, cell_budget=1)[0]) == 23 * 22 // 2              # one segment per pair
    assert len(tdisc.plan_pairs(items, lens, cell_budget=10 ** 12)[0]) == 22                  # one per row item
    # a subset of the items, given out of order and twice: still a < b, each once
    seg_a, seg_start, pair_b, pair_a = tdisc.plan_pairs([9, 3, 20, 3], lens)
    assert list(zip(pair_a.tolist(), pair_b.tolist())) == [(3, 9), (3, 20), (9, 20)]
    for few in ([], [4]):
        seg_a, seg_start, pair_b, pair_a = tdisc.plan_pairs(few, lens)
        assert len(seg_a) == len(pair_b) == len(pair_a) == 0 and seg_start.tolist() == [0]


# --------------------------------------------------------------------------- host-side scoring
def test_fragment_phones_rules():
    #          0  1  2  3  4  5  6  7  8  9 10 11 12 13 14 15 16
    labels = [5, 5, 5, 5, 5, 5, 5, 5, 2, 2, 2, 2, 7, 7, 9, 9, 9]
    # frames 6 .. 13: run 5 (8 frames) overlaps by 2 -> neither 3 frames nor half: out; run 2 whole: in; run 7 whole: in
    assert tdisc.fragment_phones(labels, 6, 13) == [2, 7]
    # frames 5 .. 12: run 5 overlaps by 3 frames (of 8: not half): the 3-frame rule decides; run 7 overlaps by 1 of 2: the half rule
    assert tdisc.fragment_phones(labels, 5, 12) == [5, 2, 7]
    # frames 9 .. 14: run 2 overlaps by 3; run 7 whole; run 9 by 1 of 3: out
    assert tdisc.fragment_phones(labels, 9, 14) == [2, 7]
    # frames 10 .. 11: run 2 overlaps by 2 of 4: the half rule decides alone
    assert tdisc.fragment_phones(labels, 10, 11) == [2]
    assert tdisc.fragment_phones(labels, 11, 11) == []                                         # 1 of 4
    assert tdisc.fragment_phones(labels, 0, 16) == [5, 2, 7, 9]
    assert tdisc.fragment_phones(labels, 40, 50) == [] and tdisc.fragment_phones([], 0, 5) == []
    assert tdisc.fragment_phones(labels, 14, 400) == [9]                                       # a span past the labels


def _levenshtein(a, b):
    row = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        new = [i]
        for j, y in enumerate(b, 1):
            new.append(min(row[j] + 1, new[j - 1] + 1, row[j - 1] + (x != y)))
        row = new
    return row[-1]


def test_ned_and_coverage_against_the_fraction_statement():
    rng = np.random.default_rng(11)
    n_frames = {f"u{k}": int(rng.integers(60, 120)) for k in range(5)}
    labels = {}
    for name, n in n_frames.items():
        row = []
        while len(row) < n:
            row += [int(rng.integers(0, 6))] * int(rng.integers(1, 9))
        labels[name] = row[:n]
    del labels["u4"]                                                # an unlabelled file
    matches = []
    for _ in range(12):
        fa, fb = rng.choice(5, 2, replace=False)
        sa, sb = int(rng.integers(0, 50)), int(rng.integers(0, 50))
        matches.append((f"u{fa}", sa, sa + int(rng.integers(0, 30)), f"u{fb}", sb, sb + int(rng.integers(0, 30))))
    matches.append(("u0", 3, 3, "u1", 7, 7))                        # single frames: most likely two empty transcriptions
    labelled = [m for m in matches if m[0] in labels and m[3] in labels]
    seqs = [(tdisc.fragment_phones(labels[m[0]], m[1], m[2]), tdisc.fragment_phones(labels[m[3]], m[4], m[5])) for m in labelled]
    lev = [_levenshtein(a, b) for a, b in seqs]
    distances, at = [], 0
    for m in matches:                                               # one per match; the unlabelled ones are never looked at
        if m[0] in labels and m[3] in labels:
            distances.append(lev[at])
            at += 1
        else:
            distances.append(10 ** 6)
    got = tdisc.scores(matches, labels, n_frames, distances=distances)
    parts = [Fraction(d, max(len(a), len(b))) for (a, b), d in zip(seqs, lev) if a or b]
    n_empty = sum(1 for a, b in seqs if not a and not b)
    assert n_empty >= 1 and len(parts) >= 5 and any(parts)
    want_ned = sum(parts) / len(parts)
    assert abs(Fraction(got["ned"]) - want_ned) <= 4 * Fraction(2.0 ** -53) * want_ned
    covered = set()
    for fa, sa, ea, fb, sb, eb in matches:
        covered |= {(fa, t) for t in range(sa, min(ea, n_frames[fa] - 1) + 1)} | {(fb, t) for t in range(sb, min(eb, n_frames[fb] - 1) + 1)}
    total = sum(n_frames.values())
    assert (got["covered_frames"], got["total_frames"]) == (len(covered), total) and got["coverage"] == len(covered) / total
    assert got["n_matches"] == 13 and got["n_ned_pairs"] == len(parts) and got["n_empty_pairs"] == n_empty
    assert got["n_unlabelled_pairs"] == 13 - len(labelled) >= 1
    assert got["n_files_with_fragment"] == len({f for f, _t in covered}) and got["n_files"] == 5
    lengths = [e - s + 1 for m in matches for s, e in ((m[1], m[2]), (m[4], m[5]))]
    assert got["mean_fragment_frames"] == math.fsum(lengths) / len(lengths)
    none = tdisc.scores([], labels, n_frames, distances=[])
    assert math.isnan(none["ned"]) and none["coverage"] == 0.0 and none["n_matches"] == 0


def test_select_orders_by_score_then_pair_index():
    score = np.array([0.5, 2.0, np.nan, 2.0, 0.0, 1.0, 2.0, 3.0], dtype=np.float32)
    span = np.array([[0, 29, 0, 29, 30], [5, 34, 0, 40, 41], [-1] * 5, [0, 24, 10, 34, 25], [-1] * 5, [0, 23, 0, 40, 41],
                     [1, 30, 2, 31, 30], [0, 40, 0, 3, 41]], dtype=np.int32)
    assert tdisc.select(score, span, 25, 0.0).tolist() == [1, 3, 6, 0]          # 5: a side of 24 frames; 7: a side of 4
    assert tdisc.select(score, span, 25, 1.0).tolist() == [1, 3, 6]
    assert tdisc.select(score, span, 1, 0.0).tolist() == [7, 1, 3, 6, 5, 0]
    assert tdisc.select(score, span, 0, 0.0).tolist() == [7, 1, 3, 6, 5, 0]     # no positive cell, not computable: never kept
    assert tdisc.select(score[:0], span[:0], 25, 0.0).tolist() == []


# --------------------------------------------------------------------------- the command line's refusals
def _argv(tmp_path, load="from_pre_computed", **kw):
    """A command line whose data directory does not exist: reading any audio or feature file would fail on its own."""
    opts = {"--threshold": "q5", "--out": str(tmp_path / "out")}
    opts.update(kw)
    argv = [load] + ([str(tmp_path / "no.pt")] if load == "from_checkpoint" else []) + [str(tmp_path / "no_such_dir")]
    for k, v in opts.items():
        argv += [k, str(v)]
    return argv


def test_refusals_before_any_file_is_opened(tmp_path):
    def refuse(kind, match, load="from_pre_computed", **kw):
        with pytest.raises(kind, match=match):
            tool.main(_argv(tmp_path, load, **kw))

    refuse(NotImplementedError, r"--file_extension \.mp3", **{"--file_extension": ".mp3"})
    refuse(NotImplementedError, r"--file_extension \.mp3", load="from_checkpoint", **{"--file_extension": ".mp3"})
    refuse(ValueError, r"--file_extension \.wav", **{"--file_extension": ".wav"})
    full = tmp_path / "full"
    full.mkdir()
    (full / "kept.txt").write_text("x")
    refuse(ValueError, "--out", **{"--out": full})
    for bad in ("abc", "q", "q0", "q100", "qx", "0", "-0.2", "nan", "inf", "q-5", ""):
        refuse(ValueError, "--threshold", **{"--threshold": bad})
    refuse(ValueError, "--gap_penalty -0.1", **{"--gap_penalty": -0.1})
    refuse(ValueError, "--gap_penalty nan", **{"--gap_penalty": "nan"})
    refuse(ValueError, "--min_frames -1", **{"--min_frames": -1})
    refuse(ValueError, "--min_score -0.5", **{"--min_score": -0.5})
    refuse(ValueError, "--max_frames 32768", **{"--max_frames": 32768})
    refuse(ValueError, "--max_frames 0", **{"--max_frames": 0})
    refuse(ValueError, "--top 0", **{"--top": 0})
    assert not os.path.exists(tmp_path / "out") and os.listdir(full) == ["kept.txt"]
    # the accepted command lines get past the refusals (and then need a GPU or, with one, the directory)
    args = tool.check_args(tool.parse_args(_argv(tmp_path)))
    assert (args.threshold_kind, args.threshold_value) == ("percentile", 5.0) and args.gap_penalty is None and args.min_frames == 25
    args = tool.check_args(tool.parse_args(_argv(tmp_path, **{"--threshold": "0.3", "--max_frames": 32767, "--gap_penalty": 0})))
    assert (args.threshold_kind, args.threshold_value) == ("value", 0.3)
    assert tool.check_args(tool.parse_args(_argv(tmp_path, load="from_checkpoint"))).file_extension == ".flac"


# --------------------------------------------------------------------------- ABI
def test_abi_names_version_and_scratch_query():
    header = open(os.path.join(ROOT, "include", "cpc2_hip.h")).read()
    assert re.search(r"\*\s*130 = cpc_local_align", header)                    # the version's line in the header comment
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("cpc_local_align_scratch_bytes", "cpc_local_align"):
        decl = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name         # the header's argument count
    assert len(_lib.SIGNATURES["cpc_local_align"][1]) == 19
    lib = _lib.load()
    assert lib.cpc_version() >= 130
    for max_len_a in (1, 63, 64):
        assert lib.cpc_local_align_scratch_bytes(100, max_len_a, 5000) == 0
    for n_seg, max_len_a, max_len_b in ((1, 65, 1), (10, 65, 500), (10, 4000, 1500), (100_000, 129, 300)):
        groups = min(n_seg, 8192)                                  # one boundary row pair per workgroup of the launch
        assert lib.cpc_local_align_scratch_bytes(n_seg, max_len_a, max_len_b) == groups * 2 * 12 * max_len_b
    for bad in ((-1, 65, 500), (10, -65, 500), (10, 65, -500)):
        lib.cpc_local_align_scratch_bytes(10, 65, 500)
        assert lib.cpc_local_align_scratch_bytes(*bad) == 0
        assert lib.cpc_last_error().startswith(b"local_align: negative size"), lib.cpc_last_error()
    assert tdisc.MAX_FRAMES == 32767 and tool.MAX_FRAMES_DEFAULT <= tdisc.MAX_FRAMES
