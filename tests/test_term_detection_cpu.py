"""Query-by-example term detection without a GPU: the definition (tests/sdtw_oracle.py) on hand-made matrices and on
planted spans, the scores of cpc2_amd.term_detection.metrics against a fractions.Fraction statement, the planner, the
refusals of the command line, and the two ABI names with the scratch query."""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from cpc2_amd import _lib
from cpc2_amd import term_detection as td
from cpc2_amd.eval import term_detection as tool
from tests import sdtw_oracle as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53                                                   # unit roundoff of float64


# --------------------------------------------------------------------------- the definition
def test_hand_made_matrices():
    # a 1 x m query takes the argmin frame, the first among equals
    assert S.sdtw([[3.0, 1.0, 2.0, 1.0]])[:4] == (1.0, 1, 1, 1)
    # an n x 1 document sums its column: the path goes straight up
    assert S.sdtw([[1.0], [2.0], [4.0]])[:4] == (7.0 / 3.0, 0, 0, 3)
    # a three-way tie takes diag.  Cell (1, 2) sees diag (0, 1), left (1, 1) and up (0, 2) at cost 1 each; the only cheap way
    # to the last row goes through it, to (2, 3): through diag the path has start 1 and length 3 (left: length 4, up: start 2)
    d = [[9.0, 1.0, 1.0, 9.0], [9.0, 0.0, 0.0, 9.0], [9.0, 9.0, 9.0, 0.0]]
    score, start, end, length, clear = S.sdtw(d)
    assert (score, start, end, length) == (1.0 / 3.0, 1, 3, 3)
    assert not clear                                              # ... and the tie is seen: the others have another length / start
    assert S.sdtw_f32(d) == (np.float32(1.0) / np.float32(3.0), 1, 3, 3)
    # the start is free: a low-cost diagonal in the middle of the document is found with its span
    d = np.full((3, 7), 5.0)
    d[0, 2] = d[1, 3] = d[2, 4] = 0.25
    assert S.sdtw(d) == (0.25, 2, 4, 3, True)
    # m < n: the path may go straight up
    assert S.sdtw([[1.0, 9.0], [1.0, 9.0], [1.0, 9.0]])[:4] == (1.0, 0, 0, 3)
    # left beats up on a tie between the two: cell (1, 2) sees left (1, 1) = 2 (length 2, start 0), up (0, 2) = 2 and diag 5
    assert S.sdtw([[1.0, 5.0, 2.0], [9.0, 1.0, 0.0]])[:4] == (2.0 / 3.0, 0, 2, 3)


def test_f64_and_f32_agree_on_exact_inputs():
    rng = np.random.default_rng(3)
    for n, m in [(1, 1), (1, 9), (7, 1), (5, 12), (13, 4), (30, 41)]:
        for scale in (1.0, 0.5):
            d = rng.integers(0, 4, (n, m)).astype(np.float64) * scale        # small integers / halves: every cost exact in f32
            s64 = S.sdtw(d)
            s32 = S.sdtw_f32(d)
            assert s32[1:] == s64[1:4], (n, m)
            # the quotient is one rounding in each format
            cost = s64[0] * s64[3]
            assert s32[0] == np.float32(np.float32(round(cost * 2) / 2) / np.float32(s64[3])), (n, m)


@pytest.mark.parametrize("distance", ["cosine", "euclidian"])
def test_planted_span_is_found(distance):
    """The property the definition is for: start and end within 8 frames of the planted span, in all 36 cases."""
    missed, unclear = [], 0
    for n, m, draw in S.PLANTED:
        rng = np.random.default_rng(1000 * n + m + draw)
        query, doc, first, last = S.planted_case(rng, n, m)
        if distance == "cosine":
            query, doc = S.unit_rows(query), S.unit_rows(doc)
        _score, start, end, _length, clear = S.sdtw(S.frame_distances(query, doc, distance))
        unclear += not clear
        if abs(start - first) > 8 or abs(end - last) > 8:
            missed.append((n, m, draw, start, first, end, last))
    assert not missed, missed
    assert unclear <= 3, unclear


# --------------------------------------------------------------------------- ranks and scores
def test_metrics_against_fractions():
    """Roundings performed per mean: a term k / r (1), the fsum of a query's terms (1), its division by R (1), the fsum over
    the queries (1) and the division by their number (1): a relative error of at most (1 + u)^5 - 1 < 6 u on values <= 1."""
    rng = np.random.default_rng(11)
    n_queries, n_docs = 7, 23
    pair_q, pair_doc = [], []
    for q in range(n_queries):
        for d in range(n_docs):
            if (q, d) in ((2, 5), (4, 0)):                         # excluded own-document pairs: absent, not misses
                continue
            pair_q.append(q)
            pair_doc.append(d)
    pair_q, pair_doc = np.array(pair_q), np.array(pair_doc)
    score = rng.integers(0, 6, len(pair_q)).astype(np.float32) / 4           # many tied scores
    score[rng.random(len(pair_q)) < 0.1] = np.nan                            # NaN scores: ranked last, ties by document
    relevant = rng.random(len(pair_q)) < 0.2
    relevant[pair_q == 3] = False                                            # a query with no relevant candidate
    relevant[(pair_q == 2) & (pair_doc == 6)] = True
    perm = rng.permutation(len(pair_q))                                      # the pairs in any order
    score, pair_q, pair_doc, relevant = score[perm], pair_q[perm], pair_doc[perm], relevant[perm]
    order, ranks = td.rank(torch.from_numpy(score), pair_q, pair_doc)
    # ranks: a permutation 1..n per query in the order of the plain sort
    for q in range(n_queries):
        pairs = [p for p in range(len(score)) if pair_q[p] == q]
        pairs.sort(key=lambda p: (math.isnan(score[p]), 0.0 if math.isnan(score[p]) else score[p], pair_doc[p]))
        assert [int(ranks[p]) for p in pairs] == list(range(1, len(pairs) + 1)), q
        assert [int(p) for p in order if pair_q[p] == q] == pairs, q
    got = td.metrics(ranks, pair_q, relevant, n_queries, names=[f"q{k}" for k in range(n_queries)])
    want, without = S.fraction_scores(score.tolist(), pair_q.tolist(), pair_doc.tolist(), relevant.tolist(), n_queries)
    assert without == [3] and got["without_relevant"] == ["q3"] and got["n_without_relevant"] == 1
    assert got["n_scored"] == n_queries - 1 and got["n_queries"] == n_queries
    for key, w in zip(("map", "p_at_10", "p_at_n", "mrr"), want):
        assert 0 < w <= 1
        assert abs(Fraction(got[key]) - w) <= 6 * Fraction(U) * w, (key, got[key], float(w))
    # the excluded pairs took no rank: query 2 has one candidate less
    assert (pair_q == 2).sum() == n_docs - 1 and ranks[pair_q == 2].max() == n_docs - 1


def test_metrics_known_answer():
    # one query, relevant at ranks 1, 3 and 12 of 12: AP = (1/1 + 2/3 + 3/12) / 3, P@10 = 2/10, P@N = 2/3 (ranks 1 and 3 are <= 3)
    ranks = np.arange(1, 13)
    relevant = np.isin(ranks, (1, 3, 12))
    got = td.metrics(ranks, np.zeros(12, int), relevant, 1)
    assert got["map"] == pytest.approx((1 + 2 / 3 + 3 / 12) / 3, rel=4 * U, abs=0)
    assert got["p_at_10"] == 0.2 and got["p_at_n"] == pytest.approx(2 / 3, rel=2 * U, abs=0) and got["mrr"] == 1.0
    none = td.metrics(ranks, np.zeros(12, int), np.zeros(12, bool), 1)
    assert none["n_scored"] == 0 and none["without_relevant"] == [0] and math.isnan(none["map"])


# --------------------------------------------------------------------------- planner
def _check_plan(queries, docs_of, lens, exclude, budget, plan):
    seg_q, seg_start, pair_doc, pair_q = plan
    assert seg_start[0] == 0 and seg_start[-1] == len(pair_doc) == len(pair_q) and len(seg_start) == len(seg_q) + 1
    assert (np.diff(seg_start) >= 1).all()
    want = [(k, int(d)) for k, q in enumerate(queries) for d in docs_of(k) if (q, int(d)) not in exclude]
    got = list(zip(pair_q.tolist(), pair_doc.tolist()))
    assert got == want                                             # every pair exactly once, in order; excluded pairs absent
    for s in range(len(seg_q)):
        a, b = seg_start[s], seg_start[s + 1]
        assert (np.asarray(queries)[pair_q[a:b]] == seg_q[s]).all()
        cells = int(lens[seg_q[s]]) * int(lens[pair_doc[a:b]].sum())
        assert cells <= budget or b - a == 1, (s, cells, budget)   # a pair larger than the budget is a segment of its own


def test_planner():
    rng = np.random.default_rng(5)
    n_docs = 200
    lens = np.concatenate([rng.integers(300, 1500, n_docs), rng.integers(50, 150, 6)])
    queries = list(range(n_docs, n_docs + 6))
    docs = np.arange(n_docs)
    exclude = {(queries[0], 17), (queries[3], 0), (queries[3], 199)}
    for budget in (1, 40_000, 1_000_000, 10 ** 12):
        plan = td.plan_segments(queries, docs, lens, exclude=exclude, cell_budget=budget)
        _check_plan(queries, lambda k: docs, lens, exclude, budget, plan)
    assert len(td.plan_segments(queries, docs, lens, cell_budget=10 ** 12)[0]) == 6
    assert len(td.plan_segments(queries, docs, lens, cell_budget=1)[0]) == 6 * n_docs
    # the default budget: few queries against many documents still make thousands of segments, even in cells
    seg_q, seg_start, pair_doc, pair_q = td.plan_segments(queries, docs, lens)
    assert 1024 <= len(seg_q) <= 6 * n_docs
    # one list per query
    per_query = [docs[k::2] for k in range(6)]
    plan = td.plan_segments(queries, per_query, lens, exclude=exclude, cell_budget=300_000)
    _check_plan(queries, lambda k: per_query[k], lens, exclude, 300_000, plan)
    # 50 queries against 10 000 documents fill 256 CUs several times over
    lens = np.concatenate([np.full(10_000, 800), np.full(50, 100)])
    seg_q = td.plan_segments(np.arange(10_000, 10_050), np.arange(10_000), lens)[0]
    assert 4 * 256 <= len(seg_q) <= 2 * td.TARGET_SEGMENTS
    with pytest.raises(ValueError, match="cell_budget"):
        td.plan_segments(queries, docs, lens, cell_budget=0)


# --------------------------------------------------------------------------- the command line's refusals
@pytest.fixture()
def lists(tmp_path):
    q, r = tmp_path / "Q.txt", tmp_path / "R.txt"
    q.write_text("hello doc1 0.50 1.10\nworld doc2\n")
    r.write_text("hello doc3 2.0 2.6\nworld doc1\n")
    return str(q), str(r)


def _argv(lists, tmp_path, **kw):
    """A command line whose data directory does not exist: reading any audio or feature file would fail on its own."""
    opts = {"--queries": lists[0], "--relevance": lists[1], "--out": str(tmp_path / "out")}
    opts.update(kw)
    argv = ["from_pre_computed", str(tmp_path / "no_such_dir")]
    for k, v in opts.items():
        argv += [k, str(v)]
    return argv


def test_refusals_before_any_file_is_opened(lists, tmp_path):
    def refuse(kind, match, **kw):
        with pytest.raises(kind, match=match):
            tool.main(_argv(lists, tmp_path, **kw))

    refuse(NotImplementedError, r"--file_extension \.mp3", **{"--file_extension": ".mp3"})
    with pytest.raises(NotImplementedError, match=r"--file_extension \.mp3"):
        tool.main(["from_checkpoint", str(tmp_path / "no.pt"), str(tmp_path / "no_such_dir"), "--file_extension", ".mp3",
                   "--queries", lists[0], "--relevance", lists[1], "--out", str(tmp_path / "out")])
    full = tmp_path / "full"
    full.mkdir()
    (full / "kept.txt").write_text("x")
    refuse(ValueError, "--out", **{"--out": full})
    refuse(ValueError, "--queries .*no such file", **{"--queries": tmp_path / "missing.txt"})
    refuse(ValueError, "--relevance .*no such file", **{"--relevance": tmp_path / "missing.txt"})
    for text, word in (("hello doc1 0.5\n", "fields"), ("hello\n", "fields"), ("hello doc1 a b\n", "not numbers"),
                       ("hello doc1 1.0 0.5\n", "onset < offset"), ("hello doc1 -1 0.5\n", "onset < offset"),
                       ("hello doc1 0 inf\n", "onset < offset")):
        bad = tmp_path / "bad.txt"
        bad.write_text("world doc2\n" + text)
        refuse(ValueError, "--queries .*bad.txt:2.*" + word, **{"--queries": bad})
        refuse(ValueError, "--relevance .*bad.txt:2.*" + word, **{"--relevance": bad})
    twice = tmp_path / "twice.txt"
    twice.write_text("hello doc1\nhello doc2\n")
    refuse(ValueError, "--queries .*twice.*hello", **{"--queries": twice})
    stranger = tmp_path / "stranger.txt"
    stranger.write_text("hello doc1\nbye doc2\n")
    refuse(ValueError, "--relevance .*not in --queries: bye", **{"--relevance": stranger})
    refuse(ValueError, "--feature_size 0", **{"--feature_size": 0})
    refuse(ValueError, "--feature_size -0.01", **{"--feature_size": -0.01})
    refuse(ValueError, "--top 0", **{"--top": 0})
    assert not os.path.exists(tmp_path / "out") and os.listdir(full) == ["kept.txt"]
    # the accepted command line gets past the refusals (and then needs a GPU or, with one, the directory)
    args = tool.check_args(tool.parse_args(_argv(lists, tmp_path)))
    assert args.query_rows == [("hello", "doc1", 0.5, 1.1), ("world", "doc2", None, None)]
    assert args.relevance_rows == [("hello", "doc3", 2.0, 2.6), ("world", "doc1", None, None)]


def test_query_span_on_the_feature_grid():
    assert tool.span_frames(0.50, 1.10, 400, 0.01) == (50, 109)               # ceil(49.5), floor(109.5)
    assert tool.span_frames(0.0, 9.0, 400, 0.01) == (0, 400)
    assert tool.span_frames(0.004, 0.012, 400, 0.01) == (0, 0)                # an empty query
    assert tool.iou(0.0, 1.0, 0.5, 1.5) == pytest.approx(1 / 3) and tool.iou(0.0, 1.0, 2.0, 3.0) == 0.0


# --------------------------------------------------------------------------- ABI
def test_abi_names_and_scratch_query():
    header = open(os.path.join(ROOT, "include", "cpc2_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("cpc_sdtw_scratch_bytes", "cpc_sdtw"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.cpc_version() >= 128
    for max_len_q in (1, 63, 64):
        assert lib.cpc_sdtw_scratch_bytes(100, max_len_q, 5000) == 0
    for n_seg, max_len_q, max_len_doc in ((1, 65, 1), (10, 65, 500), (10, 4000, 1500), (100_000, 129, 300)):
        nbytes = lib.cpc_sdtw_scratch_bytes(n_seg, max_len_q, max_len_doc)
        groups = min(n_seg, 8192)                                  # one boundary row pair per workgroup of the launch
        assert nbytes >= groups * 2 * 12 * max_len_doc, (n_seg, max_len_q, max_len_doc)
        assert nbytes <= 2 * groups * 2 * 12 * max_len_doc
    for bad in ((-1, 65, 500), (10, -65, 500), (10, 65, -500)):
        lib.cpc_sdtw_scratch_bytes(10, 65, 500)
        assert lib.cpc_sdtw_scratch_bytes(*bad) == 0
        assert lib.cpc_last_error().startswith(b"sdtw: negative size"), lib.cpc_last_error()
