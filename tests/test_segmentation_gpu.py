"""cpc_seg_dissimilarity / cpc_seg_boundaries (csrc/segment.hip), cpc2_amd.segmentation and cpc2_amd.eval.phone_segmentation on the
GPU against segmentation_oracle.py: stage 2 by equality on hand-made float64 d (peaks, prominences bit for bit, range, the four
counts, and 0xFF-filled buffers that come back with only the documented slots written), stage 1 within the oracle's stated bound
and bit-equal where the definition says so, both stages end to end by equality on cases the oracle's margin calls clear, and the
tool on synthetic audio."""
import json
import os

import numpy as np
import pytest
import torch

import segmentation_oracle as SO
from cpc2_amd import _lib
from cpc2_amd import audio
from cpc2_amd import segmentation as seg
from cpc2_amd._lib import check, ptr, stream_ptr
from cpc2_amd.eval import build_zeroSpeech_features as BZ
from cpc2_amd.eval import phone_segmentation as PS
from cpc2_amd.feature_loader import FeatureModule, buildFeature_device, loadModel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CKPT = os.path.join(ROOT, "tests", "golden", "ref_checkpoint", "checkpoint_7.pt")
DEV = torch.device("cuda:0")
PLATEAUS = [0, 1, 1, 0, 2, 2, 2, 1, 3, 3, 0, 1, 1]
P30 = [round(0.01 * i, 2) for i in range(1, 31)]


def _filled(n, dtype):
    """n elements whose every byte is 0xFF, on the device."""
    size = torch.empty(0, dtype=dtype).element_size()
    return torch.full((max(n, 1) * size,), 0xFF, dtype=torch.uint8, device=DEV).view(dtype)


def _is_fill(a):
    return (np.ascontiguousarray(a).view(np.uint8) == 0xFF).all()


def run_boundaries(ds, thresholds, refs=None, tol=2, limits=None, gaps=3):
    """cpc_seg_boundaries through the raw ABI on a batch of hand-made d arrays packed at distinct offsets with `gaps` unused slots
    between them, every output pre-filled with 0xFF -> per utterance the oracle-shaped dict; asserts the unwritten slots."""
    lib = _lib.load()
    lengths = np.array([len(d) + 1 if len(d) else 0 for d in ds], dtype=np.int32)      # frames: n = L - 1 (n = 0: L = 0 or 1)
    offsets = np.zeros(len(ds), dtype=np.int64)
    at = gaps
    for i, L in enumerate(lengths):
        offsets[i] = at
        at += int(L) + gaps
    total = at
    flat = np.full(total, np.nan)
    for d, o in zip(ds, offsets):
        flat[o:o + len(d)] = d
    k = len(thresholds)
    dd = torch.from_numpy(flat).to(DEV)
    od, ld = torch.from_numpy(offsets).to(DEV), torch.from_numpy(lengths).to(DEV)
    td = torch.tensor(thresholds, dtype=torch.float64, device=DEV)
    rf = ro = rc = lim = None
    total_ref = 0
    if refs is not None:
        cnt = np.array([len(r) for r in refs], dtype=np.int32)
        total_ref = int(cnt.sum())
        rf = torch.from_numpy(np.concatenate([np.asarray(r, dtype=np.int32) for r in refs] + [np.zeros(1, np.int32)])).to(DEV)
        ro = torch.from_numpy(np.concatenate([[0], np.cumsum(cnt[:-1])]).astype(np.int64)).to(DEV)
        rc = torch.from_numpy(cnt).to(DEV)
    if limits is not None:
        lim = torch.tensor(limits, dtype=torch.int32, device=DEV)
    u = len(ds)
    n_peaks, pos, status = _filled(u, torch.int32), _filled(total, torch.int32), _filled(u, torch.int32)
    prom, rng = _filled(total, torch.float64), _filled(u, torch.float64)
    counts = _filled((u + 1) * k * 4, torch.int32)                              # one utterance more: nothing is written behind
    check(lib.cpc_seg_boundaries(ptr(dd), total, ptr(od), ptr(ld), u, ptr(td), k, ptr(rf), total_ref, ptr(ro), ptr(rc), ptr(lim), tol,
                                 ptr(n_peaks), ptr(pos), ptr(prom), ptr(rng), ptr(counts), ptr(status), stream_ptr(DEV)),
          "seg_boundaries")
    n_peaks, pos, status = n_peaks.cpu().numpy(), pos.cpu().numpy(), status.cpu().numpy()
    prom, rng, counts = prom.cpu().numpy(), rng.cpu().numpy(), counts.cpu().numpy()
    assert _is_fill(counts[u * k * 4:])
    counts = counts[:u * k * 4].reshape(u, k, 4)
    written = np.zeros(total, bool)
    out = []
    for i, o in enumerate(offsets):
        m = int(n_peaks[i])
        assert 0 <= m <= max(len(ds[i]), 0)
        written[o:o + m] = True
        out.append({"status": int(status[i]), "peaks": pos[o:o + m].tolist(), "proms": prom[o:o + m].copy(), "range": rng[i],
                    "counts": counts[i].tolist()})
    assert _is_fill(pos[~written]) and _is_fill(prom[~written])                 # only the first n_peaks slots of each utterance
    assert np.array_equal(dd.cpu().numpy(), flat, equal_nan=True)               # d is left as it was
    return out


def assert_equals_oracle(got, d, thresholds, ref=None, tol=2, limit=None):
    want = SO.segment(d, thresholds, ref=ref, tol=tol, limit=limit)
    assert got["status"] == want["status"]
    assert got["peaks"] == want["peaks"], (got["peaks"], want["peaks"])
    assert np.array_equal(got["proms"], np.array(want["proms"], dtype=np.float64))          # bit for bit
    assert got["range"] == want["range"] or (np.isnan(got["range"]) and np.isnan(want["range"]))
    assert got["counts"] == [list(c) for c in want["counts"]], (got["counts"], want["counts"])
    return want


def _check(ds, thresholds, refs=None, tol=2, limits=None):
    got = run_boundaries(ds, thresholds, refs, tol, limits)
    wants = []
    for i, d in enumerate(ds):
        wants.append(assert_equals_oracle(got[i], d, thresholds, None if refs is None else list(refs[i]), tol,
                                          None if limits is None else limits[i]))
    return got, wants


# --------------------------------------------------------------------------- stage 2
def test_short_utterances_have_no_peak_until_n_is_3():
    ds = [np.zeros(0), np.array([0.5]), np.array([0.1, 0.9]), np.array([0.1, 0.9, 0.3]), np.array([0.2, 0.9, 0.3, 0.8])]
    got, _ = _check(ds, [0.0, 0.5], refs=[[], [], [1], [2], [2]], tol=0)
    assert [g["peaks"] for g in got] == [[], [], [], [1], [1]]
    assert got[3]["counts"][0] == [1, 1, 1, 1] and got[0]["range"] == 0.0 and got[1]["range"] == 0.0
    # a zero-frame and a one-frame utterance are the same to the kernel (n = 0); L = 1 through the lengths table too
    lib = _lib.load()
    outs = [_filled(1, torch.int32), _filled(4, torch.int32), _filled(4, torch.float64), _filled(1, torch.float64),
            _filled(4, torch.int32), _filled(1, torch.int32)]
    dd = torch.zeros(4, dtype=torch.float64, device=DEV)
    off, one = torch.tensor([1], device=DEV), torch.tensor([1], dtype=torch.int32, device=DEV)
    thr = torch.tensor([0.1], dtype=torch.float64, device=DEV)
    check(lib.cpc_seg_boundaries(ptr(dd), 4, ptr(off), ptr(one), 1, ptr(thr), 1, None, 0, None, None, None, 2,
                                 *[ptr(o) for o in outs], stream_ptr(DEV)), "seg_boundaries")
    assert int(outs[0]) == 0 and float(outs[3]) == 0.0 and outs[4].tolist() == [0, 0, 0, 0] and int(outs[5]) == 0
    assert _is_fill(outs[1].cpu().numpy()) and _is_fill(outs[2].cpu().numpy())


def test_plateaus_ties_and_walks():
    up, down = np.arange(40, dtype=np.float64), np.arange(40, dtype=np.float64)[::-1].copy()
    equal_peaks = np.array([0, 3, 1, 3, 2, 3, 0, 5, 4, 5, 0], dtype=np.float64)      # the walk passes peaks of its own height
    ascending = np.array([0, 1, 0.5, 2, 1.5, 3, 2.5, 4, 3.5, 5, 0], dtype=np.float64)  # every left walk reaches the start
    end_plateaus = np.array([2, 2, 2, 0, 1, 0, 3, 3, 3], dtype=np.float64)            # a plateau at each end is no peak
    ds = [np.array(PLATEAUS, dtype=np.float64), up, down, equal_peaks, ascending, end_plateaus]
    got, want = _check(ds, [0.0, 0.2, 1 / 3, 0.5, 1.0])
    assert got[0]["peaks"] == [1, 5, 8] and got[0]["proms"].tolist() == [1.0, 1.0, 3.0]
    assert got[1]["peaks"] == [] and got[2]["peaks"] == []
    assert got[3]["peaks"] == [1, 3, 5, 7, 9] and got[3]["proms"].tolist() == [3.0, 3.0, 3.0, 5.0, 5.0]
    assert got[4]["peaks"] == [1, 3, 5, 7, 9] and got[4]["proms"].tolist() == [0.5, 0.5, 0.5, 0.5, 5.0]
    assert got[5]["peaks"] == [4]


def test_threshold_equal_to_a_prominence_and_one_ulp_above():
    d = np.array([0.0, 0.3, 0.1, 0.7, 0.2, 1.0, 0.05, 0.4, 0.0])
    peaks, proms, rng = SO.peaks_and_prominences(d)
    assert rng == 1.0                                                    # p * range == p: the comparison is against p itself
    thresholds = []
    for pr in proms:
        thresholds += [float(pr), float(np.nextafter(pr, np.inf)), float(np.nextafter(pr, -np.inf))]
    got, _ = _check([d], thresholds)
    for j, pr in enumerate(proms):
        kept_at, kept_above = got[0]["counts"][3 * j][0], got[0]["counts"][3 * j + 1][0]
        assert kept_at == sum(1 for q in proms if q >= pr) and kept_above == kept_at - 1        # >= keeps it, one ulp drops it
    # a range that is not 1: the product p * range rounds once, as in the oracle
    d3 = d * 3.0 + 0.1
    _, proms3, rng3 = SO.peaks_and_prominences(d3)
    close = [float(pr / rng3) for pr in proms3] + [float(np.nextafter(pr / rng3, np.inf)) for pr in proms3]
    _check([d3], close)


@pytest.mark.parametrize("k", [1, 30, 64])
def test_threshold_counts(k):
    rng = np.random.default_rng(k)
    ds = [rng.random(90), rng.integers(0, 4, size=70).astype(np.float64)]
    thresholds = [0.05] if k == 1 else np.linspace(0.0, 0.6, k).tolist()
    refs = [sorted(rng.choice(np.arange(1, 90), size=12, replace=False).tolist()), [5, 6, 7, 30, 60]]
    got, _ = _check(ds, thresholds, refs=refs)
    assert len(got[0]["counts"]) == k


@pytest.mark.parametrize("tol", [0, 2, 1000])
def test_tolerances_and_matching_cases(tol):
    rng = np.random.default_rng(100 + tol)
    ds = [rng.random(120) for _ in range(3)]
    refs = [sorted(rng.choice(np.arange(1, 121), size=n, replace=False).tolist()) for n in (0, 15, 60)]
    _check(ds, [0.0, 0.1, 0.3, 2.0], refs=refs, tol=tol)                       # threshold 2.0: no hypothesis at all


def _with_boundaries(frames, n):
    """A d of n entries whose peaks at threshold 0.5 are exactly at frames - 1 (isolated spikes of height 1)."""
    d = np.zeros(n)
    for f in frames:
        d[f - 1] = 1.0
    return d


def test_the_statements_matching_examples():
    ds = [_with_boundaries([11, 13], 20), _with_boundaries([6], 20), _with_boundaries([4, 9, 15], 20), _with_boundaries([], 20),
          _with_boundaries([4, 9], 20)]
    refs = [[10, 12], [5, 6], [4, 9, 15], [3, 8], []]
    got, _ = _check(ds, [0.5], refs=refs, tol=1)
    assert got[0]["counts"][0] == [2, 2, 2, 2]                                 # ref [10, 12], hyp [11, 13], tol 1: 2 hits
    assert got[1]["counts"][0] == [1, 1, 1, 2]                                 # ref [5, 6], hyp [6]: 1 hit, both references near
    assert got[2]["counts"][0] == [3, 3, 3, 3] and got[3]["counts"][0] == [0, 0, 0, 0] and got[4]["counts"][0] == [2, 0, 0, 0]
    # hypotheses at frames >= the limit are dropped before they are counted
    got, _ = _check([_with_boundaries([4, 9, 15], 20)], [0.5], refs=[[4, 9]], tol=1, limits=[15])
    assert got[0]["counts"][0] == [2, 2, 2, 2]
    # no references given: the kept boundaries are still counted
    got, _ = _check([_with_boundaries([4, 9, 15], 20)], [0.5])
    assert got[0]["counts"][0] == [3, 0, 0, 0]


def test_a_batch_keeps_what_each_utterance_has_alone():
    rng = np.random.default_rng(8)
    ds = [np.zeros(0)] + [np.round(rng.random(n), 2) for n in (2, 63, 64, 299)]       # lengths 0, 3, 64, 65, 300
    refs = [[], [1], [5, 20, 40], [5, 20, 63], sorted(rng.choice(np.arange(1, 300), size=40, replace=False).tolist())]
    together, _ = _check(ds, P30, refs=refs)
    for i, d in enumerate(ds):
        alone = run_boundaries([d], P30, [refs[i]], gaps=7 + i)[0]
        for key in ("status", "peaks", "counts"):
            assert alone[key] == together[i][key]
        assert np.array_equal(alone["proms"], together[i]["proms"]) and alone["range"] == together[i]["range"]
    # a non-finite d: that utterance alone has status 2, no peak and zero counts
    bad = [d.copy() for d in ds]
    bad[3][17] = np.inf
    bad[2][0] = np.nan
    got, _ = _check(bad, P30, refs=refs)
    assert [g["status"] for g in got] == [0, 0, 2, 2, 0]
    for i in (0, 1, 4):
        assert got[i]["peaks"] == together[i]["peaks"] and got[i]["counts"] == together[i]["counts"]


def test_around_the_lds_staging_cap():
    cap = _lib.load().cpc_seg_lds_entries()
    rng = np.random.default_rng(cap)
    ds = []
    for n in (cap - 1, cap, cap + 1):
        d = np.round(rng.random(n), 3)                                         # a grid of 1e-3: plateaus and equal peaks
        d[n - 200:n - 100] = np.linspace(2.0, 3.0, 100)                        # long walks, a high plateau near the end
        d[-3:] = [5.0, 5.0, 1.0]
        ds.append(d)
    refs = [sorted(rng.choice(np.arange(1, cap - 1), size=500, replace=False).tolist()) for _ in ds]
    got, _ = _check(ds, P30, refs=refs)
    assert all(len(g["peaks"]) > cap // 8 for g in got) and all(g["peaks"][-1] == len(d) - 3 for g, d in zip(got, ds))


def test_long_utterances_read_in_place_with_thousands_of_peaks_and_references():
    """Beyond the staging cap d is read in place: 8192 and 8200 entries with a peak at every other one (4095 and 4099 peaks of
    random height, so the walks are long and the thresholds tell them apart) against 2560 and 3000 references."""
    cap = _lib.load().cpc_seg_lds_entries()
    rng = np.random.default_rng(4096)
    ds, refs = [], []
    for n_peaks, n_ref in ((4095, 2560), (4099, 3000)):
        n = 2 * n_peaks + 2                                                    # entries 1, 3, .. are peaks
        assert n > cap
        d = np.round(0.9 * rng.random(n), 2)
        d[1::2] = 1.0 + np.round(rng.random(n // 2), 2)
        d[-1] = 0.0
        ds.append(d)
        refs.append(sorted(rng.choice(np.arange(1, n), size=n_ref, replace=False).tolist()))
    got, _ = _check(ds, [0.0, 0.25, 0.5], refs=refs, tol=1)
    assert [len(g["peaks"]) for g in got] == [4095, 4099]
    assert all(g["counts"][0][0] == len(g["peaks"]) and g["counts"][2][0] < len(g["peaks"]) for g in got)


def test_boundaries_refuses_bad_arguments_by_name():
    lib = _lib.load()
    d = torch.zeros(8, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="thresholds"):
        seg.find_boundaries(d, [0], [8], [0.01] * 65)
    with pytest.raises(ValueError, match="tol"):
        seg.find_boundaries(d, [0], [8], [0.1], tol=-1)
    with pytest.raises(TypeError, match="float64"):
        seg.find_boundaries(d.float(), [0], [8], [0.1])
    assert lib.cpc_seg_boundaries(ptr(d), 8, None, None, 1, None, 1, None, 0, None, None, None, 2, None, None, None, None, None, None,
                                  stream_ptr(DEV)) == -1
    assert lib.cpc_last_error() == b"seg_boundaries: null buffer"
    res = seg.find_boundaries(d, [0], [8], [0.1])                              # the next call is intact
    assert int(res.n_peaks[0]) == 0 and int(res.status[0]) == 0
    # an utterance that leaves the buffer is status 2 and nothing of it is touched
    res = seg.find_boundaries(d, [0, 4], [4, 5], [0.1])
    assert res.status.tolist() == [0, 2] and res.n_peaks.tolist() == [0, 0]


# --------------------------------------------------------------------------- stage 1
def run_dissimilarity(xs, pad_cols=0, gaps=2):
    """cpc_seg_dissimilarity on utterances packed at distinct offsets in a NaN-filled buffer with row stride D + pad_cols; d
    pre-filled with 0xFF -> (list of d arrays, status); asserts that no other slot of d was written."""
    lib = _lib.load()
    D = xs[0].shape[1]
    ld = D + pad_cols
    lengths = np.array([len(x) for x in xs], dtype=np.int32)
    offsets, at = [], gaps
    for L in lengths:
        offsets.append(at)
        at += int(L) + gaps
    total = at
    buf = np.full((total, ld), np.nan, np.float32)
    for x, o in zip(xs, offsets):
        buf[o:o + len(x), :D] = x
    xd = torch.from_numpy(buf).to(DEV)
    od = torch.tensor(offsets, dtype=torch.int64, device=DEV)
    lend = torch.from_numpy(lengths).to(DEV)
    d, status = _filled(total, torch.float64), _filled(len(xs), torch.int32)
    check(lib.cpc_seg_dissimilarity(ptr(xd), total, ld, D, ptr(od), ptr(lend), len(xs), int(lengths.max()), ptr(d), ptr(status),
                                    stream_ptr(DEV)), "seg_dissimilarity")
    d = d.cpu().numpy()
    written = np.zeros(total, bool)
    out = []
    for x, o in zip(xs, offsets):
        n = max(len(x) - 1, 0)
        written[o:o + n] = True
        out.append(d[o:o + n].copy())
    assert _is_fill(d[~written])
    return out, status.cpu().numpy()


@pytest.mark.parametrize("D", [1, 3, 63, 64, 65, 256, 260])
def test_dissimilarity_within_the_stated_bound(D):
    """L = 0, 1, 2 and 130 in one batch, a row stride larger than D with NaN in the padding, a zero row (d = 1)."""
    rng = np.random.default_rng(D)
    xs = [rng.standard_normal((L, D)).astype(np.float32) for L in (0, 1, 2, 130)]
    xs[3][40] = 0.0
    xs[3][41:44] *= np.float32(1e-18)                                          # squared norms near 1e-36 * D: still exact products
    got, status = run_dissimilarity(xs, pad_cols=5)
    assert status.tolist() == [0, 0, 0, 0]
    bound = SO.dissimilarity_bound(D)
    worst = 0.0
    for x, d in zip(xs, got):
        want, _ = SO.dissimilarity(x)
        assert d.shape == want.shape
        if len(d):
            worst = max(worst, float(np.abs(d - want).max()))
    print(f"D = {D}: worst |d - d64| = {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound
    assert got[3][39] == 1.0 and got[3][40] == 1.0                             # both pairs of the zero row
    dense, status2 = run_dissimilarity(xs, pad_cols=0, gaps=0)                 # contiguous rows give the bits of the strided call
    assert all(np.array_equal(a, b) for a, b in zip(got, dense)) and status2.tolist() == [0, 0, 0, 0]


def test_dissimilarity_is_a_function_of_the_two_rows_alone():
    rng = np.random.default_rng(5)
    for D in (1, 36, 100, 256):
        a, b = rng.standard_normal((2, D)).astype(np.float32)
        period2 = np.stack([a, b] * 33)                                        # 66 frames: pairs (a, b) and (b, a) across waves and tiles
        aba = np.stack([a, b, a])
        got, _ = run_dissimilarity([period2, aba, rng.standard_normal((9, D)).astype(np.float32)])
        assert (got[0] == got[0][0]).all() and got[1][0] == got[1][1] and got[1][0] == got[0][0]


def test_non_finite_rows_set_status_2_and_leave_the_rest():
    rng = np.random.default_rng(6)
    D = 70
    clean = [rng.standard_normal((L, D)).astype(np.float32) for L in (50, 1, 40, 33)]
    want, status = run_dissimilarity(clean)
    assert status.tolist() == [0, 0, 0, 0]
    dirty = [x.copy() for x in clean]
    dirty[0][20, 69] = np.nan
    dirty[1][0, 3] = np.inf                                                    # a single frame: no pair, still status 2
    dirty[3][32, 0] = -np.inf                                                  # the last row
    got, status = run_dissimilarity(dirty)
    assert status.tolist() == [2, 2, 0, 2]
    assert np.array_equal(got[2], want[2])                                     # the neighbour keeps its bits
    keep = np.ones(49, bool)
    keep[19:21] = False
    assert np.isnan(got[0][~keep]).all() and np.array_equal(got[0][keep], want[0][keep])
    assert np.isnan(got[3][31]) and np.array_equal(got[3][:31], want[3][:31])
    # through the module: the second stage gives such an utterance no boundary
    x = torch.from_numpy(np.concatenate(dirty)).to(DEV)
    lengths = [len(c) for c in dirty]
    offsets = np.concatenate([[0], np.cumsum(lengths[:-1])])
    d, st = seg.frame_dissimilarity(x, offsets, lengths, return_status=True)
    res = seg.find_boundaries(d, offsets, lengths, [0.05])
    assert st.tolist() == [2, 2, 0, 2] and res.status.tolist() == [2, 0, 0, 2] and res.n_peaks[0] == 0 and res.n_peaks[2] > 0
    frames = seg.segment(x, offsets, lengths, prominence=0.05)
    assert len(frames[0]) == 0 and len(frames[3]) == 0 and len(frames[2]) == int(res.counts[2, 0, 0])


def test_module_shapes():
    rng = np.random.default_rng(9)
    x = rng.standard_normal((3, 20, 12)).astype(np.float32)
    xd = torch.from_numpy(x).to(DEV)
    batch = seg.frame_dissimilarity(xd, lengths=[20, 7, 1])
    assert batch.shape == (3, 20) and batch.dtype == torch.float64 and batch.is_cuda
    single = seg.frame_dissimilarity(xd[1, :7])
    assert single.shape == (6,) and torch.equal(single, batch[1, :6]) and torch.isnan(batch[1, 6:]).all()
    assert torch.isnan(batch[2]).all() and seg.frame_dissimilarity(xd[0, :0]).shape == (0,)
    wide = torch.from_numpy(np.concatenate([x[0], x[0]], axis=1)).to(DEV)
    assert torch.equal(seg.frame_dissimilarity(wide[:, :12]), batch[0, :19])   # a view with a row stride is read in place
    one = seg.segment(xd[0], prominence=0.1)
    many = seg.segment(xd, prominence=0.1)
    d0, _ = SO.dissimilarity(x[0])
    assert isinstance(one, np.ndarray) and np.array_equal(one, many[0]) and len(many) == 3
    if SO.margin(d0, [0.1]) > 1e-9:
        assert one.tolist() == SO.select(*SO.peaks_and_prominences(d0), 0.1)
    with pytest.raises(TypeError, match="fp32 only"):
        seg.frame_dissimilarity(xd.double())


# --------------------------------------------------------------------------- end to end
def _ar1(seed, L=400, D=36):
    rng = np.random.default_rng(seed)
    x = np.zeros((L, D))
    e = rng.standard_normal((L, D))
    x[0] = e[0]
    for t in range(1, L):
        x[t] = 0.8 * x[t - 1] + e[t]
    labels, lab = [], 0
    while len(labels) < L:
        labels += [lab] * int(rng.integers(3, 13))
        lab += 1
    return x.astype(np.float32), labels[:L]


def test_end_to_end_equals_the_oracle_on_clear_cases():
    """x_t = 0.8 x_t-1 + e_t, L = 400, D = 36, seeds 0-5, thresholds 0.01 .. 0.30: EVERY case must be clear (margin >= 1e-9, four
    orders above the arithmetic error of step 1), then the peaks and all counts equal the oracle's."""
    cases = [_ar1(seed) for seed in range(6)]
    oracle_d = [SO.dissimilarity(x)[0] for x, _ in cases]
    margins = [SO.margin(d, P30) for d in oracle_d]
    print("margins", ["%.2e" % m for m in margins])
    assert all(m >= 1e-9 for m in margins)
    refs = [SO.reference_boundaries(lab, len(lab)) for _, lab in cases]
    x = torch.from_numpy(np.concatenate([c[0] for c in cases])).to(DEV)
    lengths = [400] * 6
    offsets = [400 * i for i in range(6)]
    d, status = seg.frame_dissimilarity(x, offsets, lengths, return_status=True)
    res = seg.find_boundaries(d, offsets, lengths, P30, ref=refs, tol=2)
    assert status.tolist() == [0] * 6 and res.status.tolist() == [0] * 6
    peaks, counts, n_peaks = res.peaks.cpu().numpy(), res.counts.cpu().numpy(), res.n_peaks.cpu().numpy()
    dh = d.cpu().numpy()
    for i in range(6):
        want = SO.segment(oracle_d[i], P30, ref=refs[i], tol=2)
        assert np.abs(dh[400 * i:400 * i + 399] - oracle_d[i]).max() <= SO.dissimilarity_bound(36)
        assert peaks[400 * i:400 * i + n_peaks[i]].tolist() == want["peaks"]
        assert counts[i].tolist() == want["counts"]
        assert (peaks[400 * i + n_peaks[i]:400 * (i + 1)] == -1).all()
        frames = seg.select_boundaries(res, 0.05)[i]
        assert frames.tolist() == SO.select(want["peaks"], want["proms"], want["range"], 0.05)


# --------------------------------------------------------------------------- the tool
def _synthetic_db(tmp_path, n_files=4):
    """Short WAV files of tones that change every 50-120 ms, and frame labels that change with them."""
    rng = np.random.default_rng(42)
    db = tmp_path / "db" / "spk"
    db.mkdir(parents=True)
    names, labels = [], {}
    for i in range(n_files):
        n_frames = 150 + 37 * i                                                # 1.5 .. 2.6 s: one model call per file
        wave, lab, t, phone = [], [], 0, 0
        while t < n_frames:
            seg_frames = int(rng.integers(5, 13))
            freq = float(rng.uniform(200, 3000))
            s = np.arange(seg_frames * 160) / 16000.0
            wave.append(0.3 * np.sin(2 * np.pi * freq * s) + 0.02 * rng.standard_normal(len(s)))
            lab += [phone] * seg_frames
            t += seg_frames
            phone = (phone + 1 + int(rng.integers(0, 5))) % 9
        wave = np.concatenate(wave)[:n_frames * 160].astype(np.float32)
        name = f"utt{i}"
        audio.write_wav(str(db / f"{name}.wav"), wave[None, :], 16000)
        names.append(name)
        labels[name] = lab[:n_frames + (1 if i == 1 else 0)]                     # (one file has a label more than frames, if one is left)
    labels[names[2]] = labels[names[2]][:-2]                                   # two frames fewer: still within the mismatch
    path_labels = tmp_path / "labels.txt"
    path_labels.write_text("".join(f"{n} " + " ".join(str(v) for v in labels[n]) + "\n" for n in names))
    return str(tmp_path / "db"), names, labels, str(path_labels)


def _oracle_run(features, labels, names, prominences, tol=2):
    """{name: per-threshold counts}, n_ref and the pieces needed for the boundaries, from the features the tool extracted."""
    out = {}
    for name in names:
        x = features[name]
        d, _ = SO.dissimilarity(x)
        n_l = min(len(x), len(labels[name]))
        ref = SO.reference_boundaries(labels[name], n_l)
        out[name] = (SO.segment(d, prominences, ref=ref, tol=tol, limit=n_l), ref, n_l, SO.margin(d, prominences))
    return out


def _totals(run, names, k):
    n_ref = sum(len(run[n][1]) for n in names)
    tot = np.sum([np.array(run[n][0]["counts"][k]) for n in names], axis=0)
    return n_ref, int(tot[0]), int(tot[1]), int(tot[2]), int(tot[3])


def test_tool_end_to_end(tmp_path):
    db, names, labels, path_labels = _synthetic_db(tmp_path)
    out = tmp_path / "seg"
    res = PS.main(["from_checkpoint", CKPT, db, "--pathPhone", path_labels, "--out", str(out)])
    assert sorted(p.name for p in out.iterdir()) == ["boundaries.txt", "segmentation_log.json", "segmentation_scores.json"]
    scores = json.load(open(out / "segmentation_scores.json"))
    log = json.load(open(out / "segmentation_log.json"))
    assert set(log["seconds"]) == set(PS.STAGES) and all(v >= 0 for v in log["seconds"].values()) and log["utterances"] == 4
    assert scores["skipped"] == [] and scores["mismatched"] == [] and scores["non_finite"] == [] and len(scores["per_threshold"]) == 30
    for row in scores["per_threshold"]:
        for kind in ("strict", "lenient"):
            assert all(np.isfinite(v) for v in row[kind].values())
    # the oracle on the features the tool extracted
    model = loadModel([CKPT])[0]
    model.gAR.keepHidden = True
    maker = FeatureModule(model, False).cuda().eval()
    features = {}
    for name in names:
        model.gAR.hidden = None
        features[name] = buildFeature_device(maker, os.path.join(db, "spk", f"{name}.wav"))[0].float().cpu().numpy()
    run = _oracle_run(features, labels, names, P30)
    worst_margin = min(v[3] for v in run.values())
    print("tool: smallest margin", worst_margin)
    assert worst_margin >= 1e-9                                                # the comparison below is by equality
    for k, row in enumerate(scores["per_threshold"]):
        assert (row["n_ref"], row["n_hyp"], row["hits"], row["hyp_near"], row["ref_near"]) == _totals(run, names, k)
        n_ref, n_hyp, hits, hyp_near, ref_near = _totals(run, names, k)
        assert row["strict"] == SO.boundary_scores(n_ref, n_hyp, hits)
        assert row["lenient"] == SO.boundary_scores(n_ref, n_hyp, hyp_near, ref_hits=ref_near)
    rvals = [SO.boundary_scores(*_totals(run, names, k)[:3])["rval"] for k in range(30)]
    chosen = int(np.argmax(rvals))                                             # argmax: the first, i.e. lowest, among equals
    assert scores["chosen_index"] == chosen and scores["chosen_prominence"] == P30[chosen]
    lines = open(out / "boundaries.txt").read().splitlines()
    assert [ln.split()[0] for ln in lines] == names
    for ln, name in zip(lines, names):
        seg_o, _, n_l, _ = run[name]
        frames = SO.select(seg_o["peaks"], seg_o["proms"], seg_o["range"], P30[chosen], n_l)
        assert ln.split()[1:] == [f"{t:.2f}" for t in SO.boundary_times(frames)]
    assert res["names"] == names

    # from_pre_computed on the .npy files of build_zeroSpeech_features: the same counts
    feats = tmp_path / "npy"
    BZ.main([db, str(feats), CKPT, "--format", "npy", "--extension", ".wav"])
    out2 = tmp_path / "seg_pre"
    PS.main(["from_pre_computed", str(feats), "--file_extension", ".npy", "--pathPhone", path_labels, "--out", str(out2)])
    scores2 = json.load(open(out2 / "segmentation_scores.json"))
    assert scores2["per_threshold"] == scores["per_threshold"] and scores2["chosen_index"] == scores["chosen_index"]
    assert open(out2 / "boundaries.txt").read() == open(out / "boundaries.txt").read()

    # --pathDevSeqs: the threshold is chosen on the dev list only, the scores are reported on the rest
    dev = tmp_path / "dev.txt"
    dev.write_text(f"{names[0]}\n{names[3]}\n")
    out3 = tmp_path / "seg_dev"
    PS.main(["from_pre_computed", str(feats), "--file_extension", ".npy", "--pathPhone", path_labels, "--pathDevSeqs", str(dev),
             "--out", str(out3)])
    scores3 = json.load(open(out3 / "segmentation_scores.json"))
    dev_names, rest = [names[0], names[3]], [names[1], names[2]]
    dev_rvals = [SO.boundary_scores(*_totals(run, dev_names, k)[:3])["rval"] for k in range(30)]
    assert scores3["chosen_index"] == int(np.argmax(dev_rvals)) and scores3["chosen_on"] == "dev"
    assert scores3["dev_utterances"] == dev_names and scores3["n_utterances"] == 2
    for k, row in enumerate(scores3["per_threshold"]):
        assert (row["n_ref"], row["n_hyp"], row["hits"], row["hyp_near"], row["ref_near"]) == _totals(run, rest, k)

    # no labels: one threshold, boundaries.txt alone; a label-less utterance and a mismatched one are listed by name
    out4 = tmp_path / "seg_plain"
    PS.main(["from_pre_computed", str(feats), "--file_extension", ".npy", "--prominence", "0.05", "--out", str(out4)])
    assert [p.name for p in out4.iterdir()] == ["boundaries.txt"]
    short = tmp_path / "short_labels.txt"
    short.write_text("".join(f"{n} " + " ".join(str(v) for v in labels[n][:(100 if n == names[1] else None)]) + "\n"
                             for n in names[1:]))
    out5 = tmp_path / "seg_short"
    PS.main(["from_pre_computed", str(feats), "--file_extension", ".npy", "--pathPhone", str(short), "--out", str(out5)])
    scores5 = json.load(open(out5 / "segmentation_scores.json"))
    assert scores5["skipped"] == [names[0]] and [m["name"] for m in scores5["mismatched"]] == [names[1]]
    assert scores5["n_utterances"] == 2
