"""CPU-only checks of the segmentation definition (segmentation_oracle.py) and of the host side of cpc2_amd.segmentation and
cpc2_amd.eval.phone_segmentation: the oracle's peaks and prominences against scipy, the two-pointer matching against a brute-force
maximum matching, the scores on hand-computed totals, reference_boundaries, the tool's argument parsing and refusals, and the ABI
table."""
import itertools
import math

import numpy as np
import pytest
import torch

import segmentation_oracle as SO
from cpc2_amd import _lib
from cpc2_amd import segmentation as seg
from cpc2_amd.eval import phone_segmentation as PS

PLATEAUS = [0, 1, 1, 0, 2, 2, 2, 1, 3, 3, 0, 1, 1]


def test_the_plateau_case_by_hand():
    peaks, proms, rng = SO.peaks_and_prominences(PLATEAUS)
    assert peaks == [1, 5, 8] and proms == [1.0, 1.0, 3.0] and rng == 3.0
    assert SO.select(peaks, proms, rng, 1 / 3) == [2, 6, 9] and SO.select(peaks, proms, rng, 0.5) == [9]
    for short in ([], [1.0], [0.0, 1.0], [1.0, 0.0], [0.0, 2.0, 1.0]):
        assert SO.local_maxima(short) == ([1] if len(short) == 3 else [])      # n = 3: only the middle entry can be a peak
    assert SO.local_maxima([0.0, 1.0, 1.0]) == [] and SO.local_maxima([1.0, 1.0, 0.0]) == []      # a plateau touching an end


def test_oracle_peaks_and_prominences_equal_scipy():
    """50 random sequences, 20 over a 3-letter alphabet (plateaus, equal-height peaks) and the plateau case."""
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(11)
    cases = [rng.standard_normal(int(rng.integers(1, 200))) for _ in range(50)]
    cases += [rng.integers(0, 3, size=int(rng.integers(3, 120))).astype(np.float64) for _ in range(20)]
    cases.append(np.array(PLATEAUS, dtype=np.float64))
    for d in cases:
        want, _ = signal.find_peaks(d)
        want_prom = signal.peak_prominences(d, want, wlen=None)[0]
        peaks, proms, _ = SO.peaks_and_prominences(d)
        assert peaks == want.tolist()
        assert np.array_equal(np.array(proms, dtype=np.float64), want_prom)
        # selection by one product equals find_peaks(prominence=p) on the min-max normalised curve wherever that is unambiguous
    d = np.array(PLATEAUS, dtype=np.float64)
    kept, _ = signal.find_peaks((d - d.min()) / (d.max() - d.min()), prominence=0.5)
    assert [q + 1 for q in kept.tolist()] == SO.select(*SO.peaks_and_prominences(d), 0.5)


FRAMES = 12
POPCOUNT = np.array([bin(m).count("1") for m in range(1 << FRAMES)], dtype=np.int64)


def _positions(mask):
    return [f for f in range(FRAMES) if mask >> f & 1]


def _dilate(mask, tol):
    out = 0
    for s in range(-tol, tol + 1):
        out |= (mask << s) if s >= 0 else (mask >> -s)
    return out & ((1 << FRAMES) - 1)


def _brute_force_matching(ref_mask, hyp_masks, tol):
    """The maximum matching of one reference set against every hypothesis set by exhaustion over the subsets S of the references
    (Konig / Ore: the maximum matching is |ref| - max_S (|S| - |N(S)|), N(S) the hypotheses within tol of some element of S)."""
    ref = _positions(ref_mask)
    worst = np.zeros(len(hyp_masks), dtype=np.int64)                    # S empty
    for r in range(1, len(ref) + 1):
        for sub in itertools.combinations(ref, r):
            near = _dilate(sum(1 << f for f in sub), tol)
            worst = np.maximum(worst, r - POPCOUNT[hyp_masks & near])
    return len(ref) - worst


def _two_pointer_rows(ref, hyp_pos, hyp_cnt, tol):
    """The statement's two-pointer loop, run in step on one reference list against every hypothesis list (rows of hyp_pos)."""
    n = len(hyp_cnt)
    refp = np.array(list(ref) + [10 ** 6], dtype=np.int64)
    i, j, hits = (np.zeros(n, dtype=np.int64) for _ in range(3))
    rows = np.arange(n)
    for _ in range(2 * FRAMES):
        live = (i < len(ref)) & (j < hyp_cnt)
        r, h = refp[np.minimum(i, len(ref))], hyp_pos[rows, np.minimum(j, hyp_pos.shape[1] - 1)]
        hit = live & (np.abs(h - r) <= tol)
        skip_hyp = live & ~hit & (h < r)
        skip_ref = live & ~hit & ~(h < r)
        hits += hit
        i += hit | skip_ref
        j += hit | skip_hyp
    assert not ((i < len(ref)) & (j < hyp_cnt)).any()
    return hits


def test_two_pointer_matching_is_a_maximum_matching():
    """ALL pairs of boundary sets with at most 6 references and 6 hypotheses inside 12 frames (2510 x 2510), tol 0, 1, 2: the
    statement's two-pointer loop, run in step over every hypothesis set with numpy, equals the exhaustive maximum matching; and
    segmentation_oracle.match, the same loop on Python lists, equals it on eight seeded hypothesis sets per reference set and
    tolerance (60 240 calls) and on the statement's two examples."""
    masks = np.array([sum(1 << f for f in c) for r in range(7) for c in itertools.combinations(range(FRAMES), r)], dtype=np.int64)
    assert len(masks) == 2510
    lists = [_positions(int(m)) for m in masks]
    hyp_cnt = np.array([len(p) for p in lists], dtype=np.int64)
    hyp_pos = np.array([p + [10 ** 6] * (7 - len(p)) for p in lists], dtype=np.int64)
    rng = np.random.default_rng(3)
    for tol in (0, 1, 2):
        for k, ref in enumerate(lists):
            hits = _two_pointer_rows(ref, hyp_pos, hyp_cnt, tol)
            best = _brute_force_matching(int(masks[k]), masks, tol)
            assert np.array_equal(hits, best), (ref, tol, lists[int(np.flatnonzero(hits != best)[0])])
            for h in rng.integers(0, len(lists), size=8):
                assert SO.match(ref, lists[h], tol) == hits[h], (ref, lists[h], tol)
    assert SO.match([10, 12], [11, 13], 1) == 2 and SO.match([5, 6], [6], 1) == 1
    assert SO.counts([5, 6], [6], 1) == (1, 1, 1, 2)


def test_scores_on_hand_computed_totals():
    for fn in (SO.boundary_scores, seg.boundary_scores):
        perfect = fn(10, 10, 10)
        assert perfect == {"precision": 1.0, "recall": 1.0, "f1": 1.0, "os": 0.0, "rval": 1.0}
        nothing = fn(10, 0, 0)                       # P = R = F1 = 0, OS = -1: r1 = sqrt(2), r2 = 0
        assert (nothing["precision"], nothing["recall"], nothing["f1"], nothing["os"]) == (0.0, 0.0, 0.0, -1.0)
        assert nothing["rval"] == 1 - math.sqrt(2) / 2
        double = fn(10, 20, 10)                      # P = 1/2, R = 1, OS = 1: r1 = 1, r2 = -1 / sqrt(2)
        assert (double["precision"], double["recall"], double["os"]) == (0.5, 1.0, 1.0)
        assert double["f1"] == 2 * 0.5 / 1.5 and double["rval"] == 1 - (1 + 1 / math.sqrt(2)) / 2
        lenient = fn(10, 20, 12, ref_hits=9)
        assert (lenient["precision"], lenient["recall"]) == (0.6, 0.9)


def test_reference_boundaries():
    for fn in (SO.reference_boundaries, seg.reference_boundaries):
        assert list(fn([3] * 9, 9)) == []
        assert list(fn([0, 1, 0, 1, 0], 5)) == [1, 2, 3, 4]
        assert list(fn([0, 1, 0, 1, 0], 3)) == [1, 2]                  # n_l cuts the labels
        assert list(fn([0, 0, 1, 1, 1, 2], 6)) == [2, 5]
        assert list(fn([0, 1], 0)) == [] and list(fn([0, 1], 1)) == [] and list(fn([], 0)) == []
    assert seg.reference_boundaries([0, 1, 1], 3).dtype == np.int32


def test_margin_and_dissimilarity_of_the_oracle():
    d = np.array([0.0, 1.0, 0.5, 2.0, 0.0])
    assert SO.margin(d, [0.25]) == 0.0                                 # prom 0.5 == 0.25 * range 2
    assert SO.margin(d, [0.3]) == pytest.approx(0.1)
    x = np.array([[1, 0], [0, 1], [0, 0], [2, 0], [np.nan, 1], [1, 1]], np.float32)
    got, status = SO.dissimilarity(x)
    assert status == 2 and got[0] == 1.0 and got[1] == 1.0 and got[2] == 1.0 and np.isnan(got[3]) and np.isnan(got[4])
    a = np.array([[1, 2, 3], [3, 2, 1], [1, 2, 3]], np.float32)
    got, status = SO.dissimilarity(a)
    assert status == 0 and got[0] == got[1]
    assert SO.dissimilarity_bound(64) == (4 * 64 + 9) * 2.0 ** -53


# --------------------------------------------------------------------------- the tool's arguments
def _args(tmp_path, *extra, load="from_checkpoint"):
    head = [load] + (["ckpt.pt", "db"] if load == "from_checkpoint" else ["feats"])
    return PS.parse_args(head + ["--out", str(tmp_path / "out")] + list(extra))


def test_tool_arguments_and_defaults(tmp_path):
    args = PS.check_args(_args(tmp_path, "--pathPhone", "labels.txt"))
    assert args.prominence == [round(0.01 * i, 2) for i in range(1, 31)] and args.tolerance == 2
    assert args.max_length_mismatch == 2 and args.feature_size == 0.01 and args.file_extension == ".wav"
    assert not args.get_encoded and not args.seq_norm and not args.strict and args.max_size_seq == 64000 and args.level_gru is None
    args = PS.check_args(_args(tmp_path, "--prominence", "0.2", "0.05", "--pathPhone", "l", "--file_extension", ".npy",
                               "--pathSeqs", "a", "--pathDevSeqs", "b", "--tolerance", "3", load="from_pre_computed"))
    assert args.prominence == [0.05, 0.2] and args.file_extension == ".npy" and args.tolerance == 3 and args.pathDevSeqs == "b"
    assert PS.check_args(_args(tmp_path, "--prominence", "0.1")).prominence == [0.1]        # no labels: one threshold
    with pytest.raises(SystemExit):
        PS.parse_args(["--out", "x"])
    with pytest.raises(SystemExit):
        PS.parse_args(["from_pre_computed", "feats"])                   # --out is required
    with pytest.raises(SystemExit):
        _args(tmp_path, "--file_extension", ".fea", load="from_pre_computed")


def test_tool_refusals_name_their_flag(tmp_path):
    with pytest.raises(NotImplementedError, match=r"--file_extension \.mp3"):
        PS.check_args(_args(tmp_path, "--file_extension", ".mp3", "--pathPhone", "l"))
    with pytest.raises(ValueError, match="--prominence: 2 thresholds without --pathPhone"):
        PS.check_args(_args(tmp_path, "--prominence", "0.1", "0.2"))
    with pytest.raises(ValueError, match="--prominence"):
        PS.check_args(_args(tmp_path))                                  # no labels and no threshold at all
    many = [str(0.001 * i) for i in range(1, 66)]
    with pytest.raises(ValueError, match="--prominence: 65 thresholds; at most 64"):
        PS.check_args(_args(tmp_path, "--pathPhone", "l", "--prominence", *many))
    with pytest.raises(ValueError, match="--feature_size 0.02"):
        PS.check_args(_args(tmp_path, "--pathPhone", "l", "--feature_size", "0.02"))
    assert PS.check_args(_args(tmp_path, "--prominence", "0.1", "--feature_size", "0.02")).feature_size == 0.02
    with pytest.raises(ValueError, match="--pathDevSeqs"):
        PS.check_args(_args(tmp_path, "--prominence", "0.1", "--pathDevSeqs", "dev"))
    out = tmp_path / "out"
    out.mkdir()
    PS.check_args(_args(tmp_path, "--pathPhone", "l"))                  # an empty directory is fine
    (out / "old.txt").write_text("x")
    with pytest.raises(ValueError, match="--out .* not an empty directory"):
        PS.check_args(_args(tmp_path, "--pathPhone", "l"))
    # the refusal comes before any audio is read: main() with a dataset that does not exist still names --out
    with pytest.raises(ValueError, match="--out"):
        PS.main(["from_checkpoint", "missing.pt", str(tmp_path / "no_such_db"), "--pathPhone", "l", "--out", str(out)])


def test_tool_picks_the_lowest_threshold_among_equals():
    rows = [{"strict": {"rval": v}} for v in (0.2, 0.7, 0.7, 0.5)]
    assert PS.choose(rows) == 1
    assert PS.format_time(35) == "0.35" and PS.format_time(1234) == "12.34"


def test_abi_lists_the_segmentation_entry_points():
    for name in ("cpc_seg_dissimilarity", "cpc_seg_boundaries", "cpc_seg_lds_entries"):
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.cpc_version() >= 124 and 1 <= lib.cpc_seg_lds_entries() <= 8192
    # bad arguments are refused by name before any launch (no device is touched), and the next call is intact
    assert lib.cpc_seg_dissimilarity(None, 0, 4, 0, None, None, 1, 0, None, None, None) == -1
    assert lib.cpc_last_error().startswith(b"seg_dissimilarity:")
    assert lib.cpc_seg_boundaries(None, 0, None, None, 1, None, 65, None, 0, None, None, None, 2, None, None, None, None, None, None,
                                  None) == -1
    assert lib.cpc_last_error().startswith(b"seg_boundaries:") and b"k=65" in lib.cpc_last_error()
    assert lib.cpc_seg_boundaries(None, 0, None, None, 1, None, 1, None, 0, None, None, None, -1, None, None, None, None, None, None,
                                  None) == -1 and b"tol=-1" in lib.cpc_last_error()
    assert lib.cpc_seg_lds_entries() > 0


def test_no_cpu_fallback():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        seg.frame_dissimilarity(torch.zeros(5, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        seg.find_boundaries(torch.zeros(4, dtype=torch.float64), [0], [4], [0.1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        seg.segment(torch.zeros(5, 4))
