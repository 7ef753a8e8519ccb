"""Query-by-example term detection on the MI355X: cpc_sdtw against the definition (tests/sdtw_oracle.py), the work lists the
planner makes, and the command line end to end.

Exact family: frames whose distances and running costs are exact in f32 (small integers in one column under the euclidian
distance, one-hot rows under the cosine distance: 0 or 0.5).  Score bits, start, end and length EQUAL the f32 statement on
every pair, ties included.

Real-valued family: Gaussian frames.  Integers and score are compared on CLEAR pairs (sdtw_oracle: no predecessor within 1e-5
relative of the chosen one with another length or start, no other end column within 1e-5 of the best), and at most 10 % of the
pairs may be unclear.  Measured with the committed oracle alone, on the CPU: 2 of 72 pairs unclear with the cosine distance, 0
of 72 with the euclidian; 0 of 36 in the speech-like planted family."""
import json
from fractions import Fraction

import numpy as np
import pytest
import torch

from cpc2_amd import _lib
from cpc2_amd import term_detection as td
from cpc2_amd.eval import term_detection as tool
from cpc2_amd.eval.ABX import abx_iterators as abx_it
from tests import sdtw_oracle as S

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CAP = 8192                                                    # workgroups per launch
EXACT_N = (1, 2, 63, 64, 65, 128, 129, 193)                   # up to four strips
EXACT_M = (1, 2, 63, 64, 65, 127, 130, 257)
REAL_N = (1, 2, 5, 31, 63, 64, 65, 100, 129)
REAL_M = (1, 7, 63, 64, 65, 130, 200, 300)


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


def _all_pairs(queries, docs, distance, dp, gap=0, cell_budget=None):
    """Every query against every document through subsequence_dtw: score [Q, D] f32 and span [Q, D, 3], on the host."""
    frames, off, lens, lens_host = _pack(list(docs) + list(queries), dp, gap)
    nd = len(docs)
    score, span, pair_q, pair_doc = td.subsequence_dtw(frames, off, lens, np.arange(nd, nd + len(queries)), np.arange(nd), distance,
                                                       lens_host=lens_host, cell_budget=cell_budget)
    assert np.array_equal(pair_q, np.repeat(np.arange(len(queries)), nd)) and np.array_equal(pair_doc, np.tile(np.arange(nd), len(queries)))
    return score.cpu().numpy().reshape(len(queries), nd), span.cpu().numpy().reshape(len(queries), nd, 3)


def _exact_items(rng, n, distance):
    if distance == "euclidian":                               # |a - b| of small integers in column 0: dp = 4
        v = np.zeros((n, 4), dtype=np.float32)
        v[:, 0] = rng.integers(-3, 4, n)
        return v
    v = np.zeros((n, 4), dtype=np.float32)                    # one-hot rows: the distance is 0 or acos(0) / pi = 0.5
    v[np.arange(n), rng.integers(0, 4, n)] = 1.0
    return v


def _real_items(rng, n, distance):
    if distance == "cosine":                                  # 35 drawn columns + the singularity column: dp = 36
        v = torch.from_numpy(rng.standard_normal((n, 35)).astype(np.float32))
        return abx_it.normalize_with_singularity(v).numpy()
    return rng.standard_normal((n, 33)).astype(np.float32)    # dp = 36, three columns of padding


# --------------------------------------------------------------------------- exact family
@pytest.fixture(scope="module", params=["euclidian", "cosine"])
def exact(request):
    distance = request.param
    rng = np.random.default_rng(17 if distance == "cosine" else 16)
    queries = [_exact_items(rng, n, distance) for n in EXACT_N]
    docs = [_exact_items(rng, m, distance) for m in EXACT_M]
    want = [[S.sdtw_f32(S.frame_distances(q, d, distance)) for d in docs] for q in queries]
    return distance, queries, docs, want


def _assert_exact(score, span, want):
    for i, row in enumerate(want):
        for j, (v, start, end, length) in enumerate(row):
            assert type(v) is np.float32
            assert score[i, j].tobytes() == v.tobytes(), (i, j, score[i, j], v)
            assert tuple(span[i, j]) == (start, end, length), (i, j, span[i, j], (start, end, length))


def test_exact_family_equals_the_f32_statement(exact):
    distance, queries, docs, want = exact
    score, span = _all_pairs(queries, docs, distance, 4)
    _assert_exact(score, span, want)


def test_split_lists_gaps_and_repeat_give_the_same_bits(exact):
    """One query's list in one segment, in one segment per pair and in the default plan; items packed with NaN rows between
    them; the same launch twice."""
    distance, queries, docs, want = exact
    base = _all_pairs(queries, docs, distance, 4)
    for kwargs in ({"cell_budget": 10 ** 12}, {"cell_budget": 1}, {"cell_budget": 20_000}, {"gap": 3}, {}):
        other = _all_pairs(queries, docs, distance, 4, **kwargs)
        assert base[0].tobytes() == other[0].tobytes() and np.array_equal(base[1], other[1]), kwargs
    _assert_exact(*_all_pairs(queries, docs, distance, 4, gap=5, cell_budget=10 ** 12), want)


@pytest.mark.parametrize("distance", ["euclidian", "cosine"])
def test_planted_exact_copy(distance):
    """A query that is an exact copy of frames o .. o + n - 1 of the document: score 0, that span, length n.  No two
    neighbouring frames are equal, so only a diagonal has cost 0."""
    rng = np.random.default_rng(23)
    queries, docs, spans = [], [], []
    for n, m in ((1, 40), (20, 130), (64, 200), (65, 257), (129, 300), (193, 193)):
        doc = _exact_items(rng, m, distance)
        for j in range(1, m):
            while np.array_equal(doc[j], doc[j - 1]):
                doc[j] = _exact_items(rng, 1, distance)[0]
        o = int(rng.integers(0, m - n + 1))
        if n == 1:                                            # a single frame: its first occurrence wins
            o = min(j for j in range(m) if np.array_equal(doc[j], doc[o]))
        queries.append(doc[o:o + n].copy())
        docs.append(doc)
        spans.append((o, o + n - 1, n))
    score, span = _all_pairs(queries, docs, distance, 4)
    for k, want in enumerate(spans):
        assert score[k, k] == 0.0 and tuple(span[k, k]) == want, (k, score[k, k], span[k, k], want)
        assert tuple(span[k, k]) == S.sdtw_f32(S.frame_distances(queries[k], docs[k], distance))[1:]


# --------------------------------------------------------------------------- real-valued family
def _assert_clear_pairs(score, span, table, cap=0.10):
    unclear = 0
    for i, row in enumerate(table):
        for j, (v, start, end, length, clear) in enumerate(row):
            print(f"pair {i} {j}: kernel {score[i, j]!r} {tuple(span[i, j])} definition {v!r} {(start, end, length)} clear {clear}")
            if not clear:
                unclear += 1
                continue
            assert tuple(span[i, j]) == (start, end, length), (i, j, span[i, j], (start, end, length))
            assert abs(float(score[i, j]) - v) < 1e-5 * max(1.0, abs(v)), (i, j, score[i, j], v)
    n = sum(len(row) for row in table)
    assert unclear <= cap * n, (unclear, n)


@pytest.mark.parametrize("distance", ["cosine", "euclidian"])
def test_real_valued_family_on_clear_pairs(distance):
    rng = np.random.default_rng(0)
    queries = [_real_items(rng, n, distance) for n in REAL_N]
    docs = [_real_items(rng, m, distance) for m in REAL_M]
    table = [[S.sdtw(S.frame_distances(q, d, distance)) for d in docs] for q in queries]
    score, span = _all_pairs(queries, docs, distance, 36)
    _assert_clear_pairs(score, span, table)


def test_planted_spans_are_found_on_the_device():
    """The speech-like planted family in euclidian mode (its cosine dot products sit near 1, where f32 acos is the limit
    tests/test_abx_cpu.py documents): the kernel finds every span within 8 frames and agrees with the definition."""
    cases = []
    for n, m, draw in S.PLANTED:
        rng = np.random.default_rng(1000 * n + m + draw)
        cases.append(S.planted_case(rng, n, m))
    items = [c[1].astype(np.float32) for c in cases] + [c[0].astype(np.float32) for c in cases]
    frames, off, lens, lens_host = _pack(items, 16)
    k = len(cases)
    score, span, pair_q, pair_doc = td.subsequence_dtw(frames, off, lens, np.arange(k, 2 * k), [[i] for i in range(k)], "euclidian",
                                                       lens_host=lens_host)
    score, span = score.cpu().numpy(), span.cpu().numpy()
    table = []
    for i, (query, doc, first, last) in enumerate(cases):
        assert abs(span[i, 0] - first) <= 8 and abs(span[i, 1] - last) <= 8, (S.PLANTED[i], span[i], first, last)
        table.append([S.sdtw(S.frame_distances(items[k + i], items[i], "euclidian"))])
    _assert_clear_pairs(score.reshape(k, 1), span.reshape(k, 1, 3), table)


# --------------------------------------------------------------------------- work lists
@pytest.mark.parametrize("n", [3, 65])
def test_more_segments_than_the_grid_cap(n):
    """2 * 8192 + 3 segments of one pair (n = 3, m = 5): every workgroup takes a second and a third segment.  With n = 65 (two
    strips) it also reuses its boundary rows from segment to segment; they hold NaN before the launch."""
    rng = np.random.default_rng(31)
    docs = [_exact_items(rng, 5, "euclidian") for _ in range(11)]
    queries = [_exact_items(rng, n, "euclidian") for _ in range(7)]
    frames, off, lens, _ = _pack(docs + queries, 4)
    n_seg = 2 * CAP + 3
    seg_q = 11 + np.arange(n_seg) % 7
    pair_doc = (np.arange(n_seg) * 5) % 11
    nbytes = _lib.load().cpc_sdtw_scratch_bytes(n_seg, n, 5)
    assert nbytes == (CAP * 2 * 12 * 5 if n > 64 else 0)
    scratch = torch.full((max(nbytes, 1),), 0xFF, dtype=torch.uint8, device=DEV)
    score, span = td.run_segments(frames, off, lens, torch.from_numpy(seg_q.astype(np.int32)).to(DEV),
                                  torch.arange(n_seg + 1, dtype=torch.int32, device=DEV),
                                  torch.from_numpy(pair_doc.astype(np.int32)).to(DEV), n, 5, td.EUCLIDIAN, scratch=scratch)
    score, span = score.cpu().numpy(), span.cpu().numpy()
    want = {(q, d): S.sdtw_f32(S.frame_distances(queries[q], docs[d], "euclidian")) for q in range(7) for d in range(11)}
    want_score = np.array([want[(q - 11, d)][0] for q, d in zip(seg_q, pair_doc)], dtype=np.float32)
    want_span = np.array([want[(q - 11, d)][1:] for q, d in zip(seg_q, pair_doc)], dtype=np.int32)
    assert score.tobytes() == want_score.tobytes() and np.array_equal(span, want_span)


def test_boundary_rows_shared_by_the_pairs_of_a_segment_and_nan_scratch():
    """Queries of two and three strips against several documents in one segment: a workgroup's boundary rows serve one pair
    after the other.  Scratch that holds NaN before the launch changes nothing."""
    rng = np.random.default_rng(37)
    docs = [_exact_items(rng, m, "euclidian") for m in (5, 70, 130)]
    queries = [_exact_items(rng, n, "euclidian") for n in (65, 129, 3)]
    frames, off, lens, _ = _pack(docs + queries, 4)
    seg_q = torch.tensor([3, 4, 5, 4, 3], dtype=torch.int32, device=DEV)
    seg_start = torch.tensor([0, 3, 5, 8, 9, 12], dtype=torch.int32, device=DEV)
    pair_doc = torch.tensor([0, 1, 2, 2, 1, 0, 1, 2, 0, 2, 0, 1], dtype=torch.int32, device=DEV)
    nbytes = _lib.load().cpc_sdtw_scratch_bytes(5, 129, 130)
    assert nbytes == 5 * 2 * 12 * 130
    outs = []
    for fill in (0x00, 0xFF):                                  # 0xFFFFFFFF is a NaN
        scratch = torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
        score, span = td.run_segments(frames, off, lens, seg_q, seg_start, pair_doc, 129, 130, td.EUCLIDIAN, scratch=scratch)
        outs.append((score.cpu().numpy(), span.cpu().numpy()))
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and np.array_equal(outs[0][1], outs[1][1])
    seg_of_pair = np.repeat(np.arange(5), np.diff(seg_start.cpu().numpy()))
    for p, d in enumerate(pair_doc.tolist()):
        q = int(seg_q[seg_of_pair[p]]) - 3
        v, start, end, length = S.sdtw_f32(S.frame_distances(queries[q], docs[d], "euclidian"))
        assert outs[0][0][p].tobytes() == v.tobytes() and tuple(outs[0][1][p]) == (start, end, length), p


def test_uncomputable_pairs_and_bad_arguments():
    rng = np.random.default_rng(41)
    items = [_exact_items(rng, n, "euclidian") for n in (5, 70, 9, 80)]
    frames, off, lens, _ = _pack(items, 4)
    lens = lens.clone()
    lens_zero = torch.cat([lens, torch.zeros(1, dtype=torch.int32, device=DEV)])       # item 4: no frame
    off_zero = torch.cat([off, torch.zeros(1, dtype=torch.int32, device=DEV)])
    # segments: query 0 (5 frames), query 1 (70 frames), query 7 (out of range), query 4 (empty)
    seg_q = torch.tensor([0, 1, 7, 4], dtype=torch.int32, device=DEV)
    seg_start = torch.tensor([0, 4, 9, 10, 11], dtype=torch.int32, device=DEV)
    pair_doc = torch.tensor([2, -1, 3, 4, 2, 5, 1, 0, 3, 0, 0], dtype=torch.int32, device=DEV)
    lib = _lib.load()

    def edges():
        score, span = td.run_segments(frames, off_zero, lens_zero, seg_q, seg_start, pair_doc, 70, 80, td.EUCLIDIAN)
        return score.cpu().numpy(), span.cpu().numpy()

    def check_edges():
        score, span = edges()
        nan = [1, 3, 5, 9, 10]                                 # index -1, empty document, index 5, query out of range, empty query
        ok = {0: (0, 2), 2: (0, 3), 4: (1, 2), 6: (1, 1), 7: (1, 0), 8: (1, 3)}
        assert np.isnan(score[nan]).all() and (span[nan] == -1).all()
        for p, (q, d) in ok.items():
            v, start, end, length = S.sdtw_f32(S.frame_distances(items[q], items[d], "euclidian"))
            assert score[p].tobytes() == v.tobytes() and tuple(span[p]) == (start, end, length), p
        assert score[6] == 0.0                                  # an item inside itself

    check_edges()
    one = torch.zeros(16, dtype=torch.int32, device=DEV)
    rows = torch.zeros(16, dtype=torch.float32, device=DEV)
    out_score = torch.full((4,), 77.0, dtype=torch.float32, device=DEV)
    out_span = torch.full((4, 3), 77, dtype=torch.int32, device=DEV)

    def call(frames=rows, dp=4, n_items=1, n_seg=1, max_lq=4, max_ld=4, distance=td.COSINE, score=out_score, span=out_span, seg_q=one):
        return lib.cpc_sdtw(_lib.ptr(frames), dp, _lib.ptr(one), _lib.ptr(one), n_items, _lib.ptr(seg_q), _lib.ptr(one), _lib.ptr(one),
                            n_seg, max_lq, max_ld, distance, _lib.ptr(score), _lib.ptr(span), None, 0, _lib.stream_ptr(DEV))

    for kwargs, word in (({"dp": 6}, "multiple of 4"), ({"dp": 0}, "multiple of 4"), ({"dp": -4}, "multiple of 4"),
                         ({"distance": 2}, "unknown distance"), ({"distance": -1}, "unknown distance"),
                         ({"frames": None}, "null buffer"), ({"score": None}, "null buffer"), ({"span": None}, "null buffer"),
                         ({"seg_q": None}, "null buffer"), ({"n_items": 0}, "bad sizes"), ({"n_seg": -1}, "bad sizes"),
                         ({"max_ld": 0}, "bad sizes"), ({"max_lq": 0}, "bad sizes"), ({"max_lq": 65}, "scratch")):
        status = call(**kwargs)
        assert status == -1, kwargs                              # CPC_ERR_INVALID
        assert word in lib.cpc_last_error().decode(), (kwargs, lib.cpc_last_error())
        with pytest.raises(ValueError, match=word):
            _lib.check(status, "cpc_sdtw")
    assert call(n_seg=0) == 0                                    # nothing to do: OK, and nothing written
    torch.cuda.synchronize()
    assert (out_score == 77.0).all() and (out_span == 77).all()  # every refusal left the outputs untouched
    check_edges()                                                # a refusal leaves the next valid call intact
    assert lib.cpc_sdtw_scratch_bytes(20000, 65, 500) == lib.cpc_sdtw_scratch_bytes(CAP, 65, 500) == CAP * 2 * 12 * 500
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        td.run_segments(frames.cpu(), off, lens, seg_q, seg_start, pair_doc, 70, 80, td.EUCLIDIAN)


# --------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("distance", ["euclidian", "cosine"])
def test_end_to_end_on_pre_computed_features(tmp_path, distance):
    """Six .npy documents, four queries given as spans of them; two of the queries' terms are planted (a noisy copy with frames
    dropped) in other documents.  The scores file against the ranks of the definition through the Fraction statement, the
    detections line by line, and no own-document pair."""
    rng = np.random.default_rng(101)
    protos = rng.standard_normal((12, 16))
    lengths = (150, 210, 180, 260, 140, 230)
    docs = [S.speech_like(rng, m, protos=protos) for m in lengths]
    spans = {"alpha": (0, 30, 62), "beta": (1, 100, 170), "gamma": (3, 5, 45), "delta": (5, 120, 190)}   # query: (document, frames)
    planted = {"alpha": [(2, 40), (4, 90)], "beta": [(3, 150)], "gamma": [], "delta": [(0, 70), (1, 10), (2, 100)]}
    relevance = []
    for qid, places in planted.items():
        src, a, b = spans[qid]
        for d, at in places:
            keep = np.sort(rng.choice(b - a, (b - a) - int(round(0.15 * (b - a))), replace=False))
            copy = docs[src][a + keep] + 0.05 * rng.standard_normal((len(keep), 16))
            docs[d] = np.concatenate([docs[d][:at], copy, docs[d][at + len(keep):]])[:max(lengths[d], at + len(keep))]
            relevance.append((qid, d, at, at + len(keep)))
    docs = [d.astype(np.float32) for d in docs]
    feat_dir = tmp_path / "features"
    feat_dir.mkdir()
    for i, d in enumerate(docs):
        np.save(feat_dir / f"doc{i}.npy", d)
    (tmp_path / "Q.txt").write_text("".join(f"{qid} doc{src} {a / 100:.3f} {(b + 0.7) / 100:.3f}\n" for qid, (src, a, b) in spans.items()))
    (tmp_path / "R.txt").write_text("".join(f"{qid} doc{d} {a / 100:.2f} {b / 100:.2f}\n" for qid, d, a, b in relevance))
    out = tmp_path / "out"
    res = tool.main(["from_pre_computed", str(feat_dir), "--file_extension", ".npy", "--queries", str(tmp_path / "Q.txt"),
                     "--relevance", str(tmp_path / "R.txt"), "--out", str(out), "--distance_mode", distance, "--top", "4"])
    scores = json.load(open(out / "term_detection_scores.json"))
    log = json.load(open(out / "term_detection_log.json"))
    assert set(log["seconds"]) == set(tool.STAGES) and log["documents"] == 6 and log["queries"] == 4 and log["pairs"] == 20

    # the definition on the rows the tool searched
    if distance == "cosine":
        rows = [abx_it.normalize_with_singularity(torch.from_numpy(d.copy())).numpy() for d in docs]
    else:
        rows = docs
    qids = list(spans)
    score, pair_q, pair_doc, relevant, table = [], [], [], [], {}
    rel_set = {(qid, d) for qid, d, _a, _b in relevance}
    for k, qid in enumerate(qids):
        src, a, b = spans[qid]
        assert tool.span_frames(float(f"{a / 100:.3f}"), float(f"{(b + 0.7) / 100:.3f}"), lengths[src], 0.01) == (a, b)
        for d in range(6):
            if d == src:
                continue                                          # the own-document pair is excluded
            table[(k, d)] = S.sdtw(S.frame_distances(rows[src][a:b], rows[d], distance))
            score.append(table[(k, d)][0])
            pair_q.append(k)
            pair_doc.append(d)
            relevant.append((qid, d) in rel_set)
    # the test's inputs separate the documents by more than the kernel's error (1e-5 relative), so the ranks are the definition's
    for k in range(4):
        vs = sorted(s for s, q in zip(score, pair_q) if q == k)
        assert min(b - a for a, b in zip(vs, vs[1:])) > 1e-4 * max(1.0, vs[-1]), (k, vs)
    if distance == "cosine":
        # no query frame is within 1 - 1e-4 of a frame of another document: acos has a slope below 1 / sqrt(2e-4) = 71 there, and
        # an f32 dot product's few ulps of 1 (2.4e-7) move a distance by less than 6e-6: the tolerance of tests/test_abx_gpu.py holds
        for k, qid in enumerate(qids):
            src, a, b = spans[qid]
            assert max(float((rows[src][a:b].astype(np.float64) @ rows[d].astype(np.float64).T).max()) for d in range(6) if d != src) < 1 - 1e-4
    want, without = S.fraction_scores(score, pair_q, pair_doc, relevant, 4)
    assert without == [2] and scores["queries_without_relevant"] == ["gamma"] and scores["n_queries_without_relevant"] == 1
    assert scores["n_queries"] == 4 and scores["n_queries_scored"] == 3 and scores["n_documents"] == 6
    assert scores["n_pairs"] == 20 and scores["n_excluded_pairs"] == 4
    for key, w in zip(("map", "p_at_10", "p_at_n", "mrr"), want):
        assert abs(Fraction(scores[key]) - w) <= 6 * Fraction(2.0 ** -53) * w, (key, scores[key], float(w))
    assert scores["args"]["distance_mode"] == distance and scores["n_relevant_pairs_with_span"] == len(relevance)
    assert 0.0 <= scores["span_iou_at_0.5"] <= 1.0
    for key in ("missing_queries", "empty_queries", "non_finite", "too_long", "relevant_missing"):
        assert scores[key] == []

    lines = [ln.split() for ln in open(out / "detections.txt").read().splitlines()]
    assert len(lines) == 4 * 4                                    # --top 4 of the 5 candidates of every query
    at = 0
    n_iou = 0
    for k, qid in enumerate(qids):
        ranked = sorted((d for d in range(6) if (k, d) in table), key=lambda d: (table[(k, d)][0], d))
        for r, d in enumerate(ranked[:4]):
            name, doc, rank_s, score_s, start_s, end_s, rel_s = lines[at]
            at += 1
            v, start, end, length, clear = table[(k, d)]
            assert (name, doc, int(rank_s), int(rel_s)) == (qid, f"doc{d}", r + 1, int((qid, d) in rel_set)), lines[at - 1]
            assert doc != f"doc{spans[qid][0]}"
            assert abs(float(score_s) - v) < 1e-5 * max(1.0, abs(v)), (lines[at - 1], v)
            if clear:
                assert (start_s, end_s) == (f"{start / 100:.2f}", f"{(end + 1) / 100:.2f}"), (lines[at - 1], start, end)
    for qid, d, a, b in relevance:                                # the share of labelled spans found, from the definition's spans
        k = qids.index(qid)
        _v, start, end, _l, _c = table[(k, d)]
        n_iou += tool.iou(start / 100, (end + 1) / 100, a / 100, b / 100) >= 0.5
    assert scores["span_iou_at_0.5"] == n_iou / len(relevance)
    assert res["scores"]["map"] == scores["map"]
    # a second run into the same directory is refused: nothing is overwritten
    with pytest.raises(ValueError, match="--out"):
        tool.main(["from_pre_computed", str(feat_dir), "--file_extension", ".npy", "--queries", str(tmp_path / "Q.txt"),
                   "--relevance", str(tmp_path / "R.txt"), "--out", str(out)])
