"""ABX on quantized units on the MI355X: cpc_abx_dtw_units against the fp64 oracle (tests/abx_oracle.py), against the dense
kernel on the one-hot expansion and against the reference's outputs in g22_abx_units.npz; the unit path of the scorer
against the golden sparse tensors and against the dense path; ClusteringFeatures against the reference's recorded tensors;
the command line end to end on the committed audio.

On one-hot frames the cosine frame distance is exactly 0 or 0.5 in f32, so every DTW cost is an exact multiple of 0.5 and
the value cost / length one correctly rounded f32 division: the cosine checks ask for equality, not closeness."""
import json
import os
import random

import numpy as np
import pytest
import torch

from cpc2_amd import _lib
from cpc2_amd.eval import eval_ABX
from cpc2_amd.eval import eval_ABX_clustering as EC
from cpc2_amd.eval.ABX import abx_group_computation as abx_g
from cpc2_amd.eval.ABX import abx_iterators as abx_it
from tests import abx_oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ITEM = os.path.join(GOLDEN, "g19_abx_synth.item")
DEV = torch.device("cuda:0")
COS, EUC = abx_g.get_cosine_distance_batch, abx_g.get_euclidian_distance_batch
VARIANTS = {"u8": ("g22_quantized_units.txt", None), "u50": ("g22_quantized_units_50.txt", None),
            "ug": ("g22_quantized_units_groups.txt", "g22_onehot_dict.txt")}


@pytest.fixture(scope="module")
def g22():
    return np.load(os.path.join(GOLDEN, "g22_abx_units.npz"), allow_pickle=False)


def _runs(rng, n, n_units):
    out = []
    while len(out) < n:
        out += [int(rng.integers(0, n_units))] * int(rng.integers(1, 6))
    return np.array(out[:n], dtype=np.int64)


def _unit_items(seqs, fn, normalize=True, n_units=None):
    n_units = n_units or int(max(int(s.max()) for s in seqs)) + 1
    lens = [len(s) for s in seqs]
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    code = abx_g._distance_code(fn)
    return abx_g._UnitItems(torch.from_numpy(np.concatenate(seqs).astype(np.int32)).to(DEV),
                            torch.from_numpy(off.astype(np.int32)).to(DEV),
                            torch.tensor(lens, dtype=torch.int32, device=DEV), lens,
                            {code: abx_g.unit_frame_distances(n_units, normalize, fn)}), code


def _all_pairs(nx, ny):
    return np.repeat(np.arange(nx), ny), np.tile(np.arange(ny), nx) + nx


def _unit_kernel(xs, ys, fn, n_units=None):
    """Value and path length of every (x, y) through cpc_abx_dtw_units."""
    items, code = _unit_items(list(xs) + list(ys), fn, n_units=n_units)
    px, py = _all_pairs(len(xs), len(ys))
    vals, plen = abx_g._dtw_pairs(items, px, py, code)
    return vals.cpu().numpy().reshape(len(xs), len(ys)), plen.cpu().numpy().reshape(len(xs), len(ys))


def _expand(u, n_units):
    """The loader's rows of one item: the one-hot row as [1, L, n_units] through normalize_with_singularity."""
    rows = torch.zeros(1, len(u), n_units)
    rows.scatter_(-1, torch.from_numpy(np.asarray(u, dtype=np.int64)).view(1, -1, 1), 1)
    return abx_it.normalize_with_singularity(rows)[0]


def _dense_kernel(xs, ys, fn, n_units):
    """The same pairs through cpc_abx_dtw on the one-hot expansion."""
    def padded(seqs):
        S = max(len(s) for s in seqs)
        out = torch.zeros(len(seqs), S, n_units + 1)
        for i, s in enumerate(seqs):
            out[i, :len(s)] = _expand(s, n_units)
        return out.to(DEV), torch.tensor([len(s) for s in seqs])
    items = abx_g._Items.from_padded([padded(xs), padded(ys)], DEV)
    px, py = _all_pairs(len(xs), len(ys))
    vals, plen = abx_g._dtw_pairs(items, px, py, abx_g._distance_code(fn))
    return vals.cpu().numpy().reshape(len(xs), len(ys)), plen.cpu().numpy().reshape(len(xs), len(ys))


def _oracle(x, y, d_same, d_diff):
    d = np.where(np.asarray(x)[:, None] == np.asarray(y)[None, :], np.float64(np.float32(d_same)),
                 np.float64(np.float32(d_diff)))
    return O.dtw(d)


X_LENS = [1, 2, 63, 64, 65, 90, 200, 7]           # short and strip-length items in one segment list
Y_LENS = [1, 2, 63, 64, 65, 90, 200, 33, 5]


@pytest.mark.parametrize("n_units", [2, 8, 2000])
def test_unit_kernel_equals_oracle_cosine(n_units):
    rng = np.random.default_rng(n_units)
    xs = [_runs(rng, n, n_units) for n in X_LENS]
    ys = [_runs(rng, n, n_units) for n in Y_LENS]
    d_same, d_diff = abx_g.unit_frame_distances(n_units, True, COS)
    assert (d_same, d_diff) == (0.0, 0.5)
    vals, plen = _unit_kernel(xs, ys, COS, n_units)
    for i, x in enumerate(xs):
        for j, y in enumerate(ys):
            v, n = _oracle(x, y, d_same, d_diff)
            assert vals[i, j] == np.float32(v), (i, j, vals[i, j], v)
            assert plen[i, j] == n, (i, j, plen[i, j], n)


@pytest.mark.parametrize("n_units", [2, 8, 2000])
def test_unit_kernel_against_oracle_euclidian(n_units):
    rng = np.random.default_rng(100 + n_units)
    xs = [_runs(rng, n, n_units) for n in X_LENS]
    ys = [_runs(rng, n, n_units) for n in Y_LENS]
    d_same, d_diff = abx_g.unit_frame_distances(n_units, True, EUC)
    assert d_same == 0.0 and d_diff == float(np.sqrt(np.float32(2.0)))
    vals, plen = _unit_kernel(xs, ys, EUC, n_units)
    for i, x in enumerate(xs):
        for j, y in enumerate(ys):
            v, n = _oracle(x, y, d_same, d_diff)
            assert abs(vals[i, j] - v) < 1e-5 * max(1.0, abs(v)), (i, j, vals[i, j], v)
            assert plen[i, j] == n, (i, j, plen[i, j], n)


@pytest.mark.parametrize("n_units", [2, 8, 50])
@pytest.mark.parametrize("dist", ["cosine", "euclidian"])
def test_unit_kernel_equals_dense_kernel_on_one_hot(n_units, dist):
    rng = np.random.default_rng(200 + n_units)
    fn = COS if dist == "cosine" else EUC
    xs = [_runs(rng, n, n_units) for n in X_LENS]
    ys = [_runs(rng, n, n_units) for n in Y_LENS]
    vals, plen = _unit_kernel(xs, ys, fn, n_units)
    dvals, dplen = _dense_kernel(xs, ys, fn, n_units)
    assert np.array_equal(plen, dplen)
    assert np.array_equal(vals, dvals), np.abs(vals - dvals).max()


def test_unit_kernel_equals_dense_kernel_2000_units():
    rng = np.random.default_rng(2000)
    xs = [_runs(rng, n, 2000) for n in (1, 65, 30)]
    ys = [_runs(rng, n, 2000) for n in (2, 64, 90)]
    vals, plen = _unit_kernel(xs, ys, COS, 2000)
    dvals, dplen = _dense_kernel(xs, ys, COS, 2000)
    assert np.array_equal(plen, dplen) and np.array_equal(vals, dvals)


def test_strip_ends_stale_boundary_columns_and_the_not_computable_rule():
    """What X_LENS / Y_LENS leave open, against the oracle bit for bit (cosine: 0 / 0.5).  x of 128 (last row in lane 63), 129
    (last row in lane 0 of a third strip) and 192 frames (three full strips) against y of 1, 64, 65, 129 and 130, the y items
    ordered so that wave w of the four takes pairs w and w + 4 of a segment: a long y and then a short one under the same
    x, whose boundary rows then hold stale columns beyond the shorter y.  Then the rule for what is not computable: with
    max_len_y = 50 and a y of 100 frames in the list, an x of one strip (64) is computed against it (no boundary row is
    touched), an x of 65 frames is NaN / -1; the scratch is of exactly the queried size and nothing is written behind it."""
    n_units = 6
    rng = np.random.default_rng(31)
    d_same, d_diff = abx_g.unit_frame_distances(n_units, True, COS)
    assert (d_same, d_diff) == (0.0, 0.5)
    xs = [_runs(rng, n, n_units) for n in (128, 129, 192)]
    ys = [_runs(rng, n, n_units) for n in (130, 129, 65, 64, 1)]
    order = [0, 1, 2, 3, 4, 3, 4, 2]                       # waves: 130 -> 1, 129 -> 64, 65 -> 1, 64 -> 65
    items, code = _unit_items(xs + ys, COS, n_units=n_units)
    px = np.repeat(np.arange(len(xs)), len(order))
    py = np.tile(np.array(order), len(xs)) + len(xs)
    vals, plen = abx_g._dtw_pairs(items, px, py, code)
    vals, plen = vals.cpu().numpy(), plen.cpu().numpy()
    want = {(i, j): _oracle(x, y, d_same, d_diff) for i, x in enumerate(xs) for j, y in enumerate(ys)}
    for p, (i, j) in enumerate(zip(px, py - len(xs))):
        v, n = want[i, j]
        assert vals[p] == np.float32(v) and plen[p] == n, (p, len(xs[i]), len(ys[j]), vals[p], v, plen[p], n)

    seqs = [_runs(rng, n, n_units) for n in (64, 65, 100, 30)]
    items, code = _unit_items(seqs, COS, n_units=n_units)
    lib = _lib.load()
    seg_x = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    seg_start = torch.tensor([0, 2, 4], dtype=torch.int32, device=DEV)
    pair_y = torch.tensor([2, 3, 2, 3], dtype=torch.int32, device=DEV)
    nbytes = lib.cpc_abx_dtw_units_scratch_bytes(2, 65, 50)
    assert nbytes == 2 * 4 * 2 * 8 * 50
    guard = 4096
    scratch = torch.full((nbytes + guard,), 0xFF, dtype=torch.uint8, device=DEV)
    vals = torch.zeros(4, dtype=torch.float32, device=DEV)
    plen = torch.zeros(4, dtype=torch.int32, device=DEV)
    _lib.check(lib.cpc_abx_dtw_units(_lib.ptr(items.units), _lib.ptr(items.off), _lib.ptr(items.lens), items.n,
                                     _lib.ptr(seg_x), _lib.ptr(seg_start), _lib.ptr(pair_y), 2, 65, 50, d_same, d_diff,
                                     _lib.ptr(vals), _lib.ptr(plen), _lib.ptr(scratch), nbytes, _lib.stream_ptr(DEV)),
               "cpc_abx_dtw_units")
    vals, plen = vals.cpu().numpy(), plen.cpu().numpy()
    assert (scratch[nbytes:] == 0xFF).all().item()
    for p, (i, j) in enumerate(((0, 2), (0, 3), (1, 2), (1, 3))):
        if (i, j) == (1, 2):                                 # 65 frames against 100 > max_len_y: a boundary row would not hold it
            assert np.isnan(vals[p]) and plen[p] == -1
        else:
            v, n = _oracle(seqs[i], seqs[j], d_same, d_diff)
            assert vals[p] == np.float32(v) and plen[p] == n, (p, vals[p], v, plen[p], n)


def test_reference_dtw_cases(g22):
    for k in range(int(g22["dtw_n"])):
        code, sym, n_units = (int(v) for v in g22[f"dtw{k}_cfg"])
        fn = COS if code == 0 else EUC
        xs = [row[row >= 0].astype(np.int64) for row in g22[f"dtw{k}_x"]]
        ys = [row[row >= 0].astype(np.int64) for row in g22[f"dtw{k}_y"]]
        vals, _ = _unit_kernel(xs, ys, fn, n_units)
        ref = g22[f"dtw{k}_out"]
        if sym:                                              # the reference computes j > i, mirrors, leaves the diagonal 0
            iu = np.triu_indices(len(xs), 1)
            assert np.array_equal(vals[iu], ref[iu]), k
            assert np.array_equal(ref.T[iu], ref[iu]) and not ref.diagonal().any()
        else:
            assert np.array_equal(vals, ref), (k, np.abs(vals - ref).max())
        # the reference-shaped entry point on the expansion (the dense kernel)
        def padded(seqs):
            S = max(len(s) for s in seqs)
            out = torch.zeros(len(seqs), S, n_units + 1)
            for i, s in enumerate(seqs):
                out[i, :len(s)] = _expand(s, n_units)
            return out.to(DEV), torch.tensor([len(s) for s in seqs])
        a, sa = padded(xs)
        b, sb = padded(ys)
        dense = abx_g.get_distance_group_dtw(a, b, sa, sb, ignore_diag=bool(sym), symmetric=bool(sym),
                                             distance_function=fn).numpy()
        assert np.array_equal(dense, ref), (k, np.abs(dense - ref).max())


def test_unit_test_answers():
    """Hand-checked: x = [0, 1, 1], y = [0, 1]: path (0,0) (1,1) (2,1), cost 0, length 3; x = [0], y = [1, 1, 0]: the
    first row, cost 2 * 0.5, length 3; x = [3], y = [3]: one cell."""
    vals, plen = _unit_kernel([np.array([0, 1, 1]), np.array([0]), np.array([3])],
                              [np.array([0, 1]), np.array([1, 1, 0]), np.array([3])], COS, 4)
    assert vals[0, 0] == 0.0 and plen[0, 0] == 3
    assert vals[1, 1] == np.float32(1.0) / np.float32(3.0) and plen[1, 1] == 3
    assert vals[2, 2] == 0.0 and plen[2, 2] == 1
    assert vals[2, 0] == np.float32(0.5) and plen[2, 0] == 2          # [3] against [0, 1]: 0.5 + 0.5 over 2


def test_out_of_range_items_and_bad_arguments():
    rng = np.random.default_rng(5)
    items, code = _unit_items([_runs(rng, n, 8) for n in (5, 70, 9)], COS, n_units=8)
    lib = _lib.load()
    # segments x = 0, 1, 7 (no such item); pairs: (0, 2) (0, 3: no such item) (0, -1) | (1, 2) (1, 1) | (7, 0)
    seg_x = torch.tensor([0, 1, 7], dtype=torch.int32, device=DEV)
    seg_start = torch.tensor([0, 3, 5, 6], dtype=torch.int32, device=DEV)
    pair_y = torch.tensor([2, 3, -1, 2, 1, 0], dtype=torch.int32, device=DEV)
    vals = torch.zeros(6, dtype=torch.float32, device=DEV)
    plen = torch.zeros(6, dtype=torch.int32, device=DEV)
    nbytes = lib.cpc_abx_dtw_units_scratch_bytes(3, 70, 70)
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    d_same, d_diff = items.distances[code]
    _lib.check(lib.cpc_abx_dtw_units(_lib.ptr(items.units), _lib.ptr(items.off), _lib.ptr(items.lens), items.n,
                                     _lib.ptr(seg_x), _lib.ptr(seg_start), _lib.ptr(pair_y), 3, 70, 70, d_same, d_diff,
                                     _lib.ptr(vals), _lib.ptr(plen), _lib.ptr(scratch), nbytes, _lib.stream_ptr(DEV)),
               "cpc_abx_dtw_units")
    vals, plen = vals.cpu().numpy(), plen.cpu().numpy()
    assert np.isnan(vals[[1, 2, 5]]).all() and (plen[[1, 2, 5]] == -1).all()
    assert not np.isnan(vals[[0, 3, 4]]).any() and (plen[[0, 3, 4]] > 0).all()
    assert vals[4] == 0.0 and plen[4] == 70                    # an item against itself: the diagonal
    one = torch.zeros(4, dtype=torch.int32, device=DEV)
    outv = torch.zeros(4, dtype=torch.float32, device=DEV)

    def call(units=one, n_items=1, max_lx=4, max_ly=4, d_same=0.0, scratch=None, nbytes=0):
        return lib.cpc_abx_dtw_units(_lib.ptr(units), _lib.ptr(one), _lib.ptr(one), n_items, _lib.ptr(one), _lib.ptr(one),
                                     _lib.ptr(one), 1, max_lx, max_ly, d_same, 0.5, _lib.ptr(outv), None,
                                     _lib.ptr(scratch), nbytes, _lib.stream_ptr(DEV))
    for kwargs, word in (({"units": None}, "null buffer"), ({"n_items": 0}, "bad sizes"), ({"max_ly": 0}, "bad sizes"),
                         ({"d_same": float("nan")}, "NaN"), ({"max_lx": 65}, "scratch")):
        with pytest.raises(ValueError, match=word):
            _lib.check(call(**kwargs), "cpc_abx_dtw_units")
    assert lib.cpc_abx_dtw_units_scratch_bytes(10, 64, 500) == 0
    assert lib.cpc_abx_dtw_units_scratch_bytes(10, 65, 500) >= 10 * 2 * 500 * 8
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- whole evaluation
def _maker(tag):
    name, dic = VARIANTS[tag]
    return EC.QuantizedClustering(os.path.join(GOLDEN, name), os.path.join(GOLDEN, dic) if dic else None)


SEQS = [(f"f{f}", f"f{f}.flac") for f in range(6)]


@pytest.mark.parametrize("tag", ["u8", "u50", "ug"])
def test_unit_path_equals_golden_and_dense_path(g22, tag):
    seed, step, msg, mxa, n_units = (int(v) for v in g22[f"{tag}_cfg"])
    qc = _maker(tag)
    assert qc.n_units == n_units
    units = abx_it.ABXUnitLoader(ITEM, SEQS, qc.unit_function, float(step), True, qc.n_units)
    dense = abx_it.ABXFeatureLoader(ITEM, SEQS, qc.feature_function, float(step), True)
    assert np.array_equal(np.array(units.features, dtype=np.float64), g22[f"{tag}_features"])
    assert units.features == dense.features
    results = {}
    for name, ds in (("units", units), ("dense", dense)):
        random.seed(seed)
        for mode in ("within", "across"):
            it = ds.get_iterator(mode, msg, mxa)
            stats = {}
            sp = abx_g.get_abx_scores_dtw_on_group(it, COS, it.symmetric, stats=stats)
            results[name, mode] = sp
            coords, values = sp._indices().numpy().T, sp._values().numpy()
            print(tag, name, mode, len(values), "triplets", stats["unique_pairs"], "pairs, max |value - golden|",
                  np.abs(values - g22[f"{tag}_{mode}_values"]).max())
            assert np.array_equal(coords, g22[f"{tag}_{mode}_coords"])
            assert np.array_equal(values, g22[f"{tag}_{mode}_values"]), (name, mode)       # the assertion that binds
    scores = np.array([eval_ABX.score_within(results["units", "within"]), eval_ABX.score_across(results["units", "across"])])
    assert np.abs(scores - g22[f"{tag}_scores"]).max() < 1e-4
    random.seed(seed)
    again = EC.eval_ABX_Librispeech("unused", ITEM, qc.feature_function, modes="all", feature_size=1 / step,
                                    unit_function=qc.unit_function, n_units=qc.n_units, seq_list=SEQS)
    assert again["within"] == scores[0] and again["across"] == scores[1]


def test_unit_store_groups_go_through_the_per_group_path(g22):
    """The reference-shaped interface on the unit store: iterating yields expanded groups that loc_dtw accepts, and gives
    what the batched unit path gives."""
    seed, step, msg, mxa, n_units = (int(v) for v in g22["u8_cfg"])
    qc = _maker("u8")
    ds = abx_it.ABXUnitLoader(ITEM, SEQS, qc.unit_function, float(step), True, qc.n_units)
    ds.cuda()
    random.seed(seed)
    it = ds.get_iterator("within", msg, mxa)
    batched = abx_g.get_abx_scores_dtw_on_group(it, COS, it.symmetric)
    random.seed(seed)
    it = ds.get_iterator("within", msg, mxa)
    coords, values = [], []
    for n, group in enumerate(it):
        if n == 12:
            break
        c, v = abx_g.loc_dtw(group, COS, it.symmetric)
        coords.append(c)
        values.append(v)
    assert np.array_equal(batched._indices().numpy().T[:12], np.array(coords))
    assert np.array_equal(batched._values().numpy()[:12], torch.FloatTensor(values).numpy())


def _synthetic_item_set(path, rng, n_files, frames):
    """Phone-like items over n_files files of `frames` frames at 100 Hz: 8 speakers, 6 phones, 3 contexts, 5-20 frames."""
    lines = ["#file onset offset #phone prev-phone next-phone speaker"]
    for f in range(n_files):
        t = 0.05
        while t < frames / 100 - 0.3:
            dur = float(rng.integers(5, 21)) / 100
            ph = "abcdef"[int(rng.integers(0, 6))]
            c = [("x", "y"), ("y", "z"), ("z", "x")][int(rng.integers(0, 3))]
            lines.append(f"s{f} {t:.3f} {t + dur:.3f} {ph} {c[0]} {c[1]} spk{f % 8}")
            t += dur + 0.01
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def test_unit_path_builds_no_dense_matrix(tmp_path):
    """2000 units over 48 000 frames: the one-hot matrix alone is 384 MB on the device (as much again on the host).  The
    unit path holds 4 bytes per frame plus the index and pair lists of a chunk (about 16 bytes per index entry; 9 MB at
    the peak here), so the bound separates the two designs, not two allocation patterns."""
    n_units, n_files, frames = 2000, 48, 1000
    rng = np.random.default_rng(77)
    item = tmp_path / "synth.item"
    _synthetic_item_set(item, rng, n_files, frames)
    units = {f"s{f}": torch.from_numpy(_runs(rng, frames, n_units)) for f in range(n_files)}
    seqs = [(k, k) for k in sorted(units)]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    random.seed(3)
    scores = EC.eval_ABX_Librispeech("unused", str(item), None, modes="all", unit_function=lambda p: units[p],
                                     n_units=n_units, seq_list=seqs)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    total_frames = n_files * frames
    print("peak device memory of the unit path:", peak, "bytes; dense matrix:", total_frames * n_units * 4)
    assert peak < total_frames * n_units * 4
    assert 0.0 <= scores["within"] <= 1.0 and 0.0 <= scores["across"] <= 1.0


# --------------------------------------------------------------------------- ClusteringFeatures
class _FakeMaker:
    def __init__(self, dim):
        self.out_feature_dim = dim


def _clustering_features(monkeypatch, tmp_path, g22, n_groups, soft, mode):
    ck = torch.from_numpy(g22["cf_Ck"])
    feat = torch.from_numpy(g22[f"cf_g{n_groups}_feat"])
    run = tmp_path / f"run_{n_groups}_{soft}_{mode}"
    run.mkdir()
    torch.save({"state_dict": {"Ck": ck}}, run / "checkpoint_last.pt")
    with open(run / "args.json", "w") as fh:
        json.dump({"pathCheckpoint": "recorded", "encoder_layer": False, "level_gru": None}, fh)
    monkeypatch.setattr(EC, "load_cpc_feature_maker", lambda *a, **k: _FakeMaker(feat.size(2)))
    monkeypatch.setattr(EC, "buildFeature", lambda fm, x, **k: feat.clone())
    cf = EC.ClusteringFeatures(str(run / "checkpoint_last.pt"), soft_clustering=soft, group_modes=mode,
                               onehot_dict=os.path.join(GOLDEN, "g22_onehot_dict.txt"))
    assert cf.n_groups == n_groups and cf.dim_clusters == ck.size(2)
    return cf, feat


@pytest.mark.parametrize("n_groups", [1, 2])
def test_clustering_features_against_the_reference(monkeypatch, tmp_path, g22, n_groups):
    cf, feat = _clustering_features(monkeypatch, tmp_path, g22, n_groups, True, "concat")
    soft = cf.feature_function("x").cpu().numpy()
    ref = g22[f"cf_g{n_groups}_soft"]
    assert soft.shape == ref.shape and not cf.has_units
    assert (np.abs(soft - ref) <= 1e-5 * np.maximum(np.abs(ref), 1e-30)).all(), np.abs(soft / ref - 1).max()
    for mode in ("seq", "onehot", "concat", "combine"):
        cf, feat = _clustering_features(monkeypatch, tmp_path, g22, n_groups, False, mode)
        out = cf.feature_function("x")
        ref = g22[f"cf_g{n_groups}_{mode}"]
        assert out.is_cuda and out.dtype == torch.float32
        assert np.array_equal(out.cpu().numpy(), ref.astype(np.float32)), mode
        assert cf.step_feature_multiplication == int(g22[f"cf_g{n_groups}_{mode}_step"])
        single = n_groups == 1 or mode in ("seq", "onehot")
        assert cf.has_units == single
        if single:
            units = cf.unit_function("x")
            assert units.dtype == torch.int64 and units.dim() == 1
            assert np.array_equal(units.cpu().numpy(), ref[0].argmax(1)) and cf.n_units == ref.shape[2]
            if not (n_groups > 1 and mode == "onehot"):
                dist = cf.clusterModule(feat.to(DEV).view(1, -1, cf.dim_clusters))
                assert torch.equal(units, dist.argmin(-1)[0])
        else:
            with pytest.raises(ValueError, match="no single unit"):
                cf.unit_function("x")


# --------------------------------------------------------------------------- end to end on the committed audio
CKPT = os.path.join(GOLDEN, "ref_checkpoint", "checkpoint_7.pt")
DB = os.path.join(GOLDEN, "test_db")
DB_ITEM = os.path.join(GOLDEN, "g19_abx_test_db.item")


def test_end_to_end_on_committed_audio(tmp_path):
    import logging
    from pathlib import Path
    from cpc2_amd.clustering import clustering_quantization as Q
    from cpc2_amd.clustering import clustering_script as S
    clust = tmp_path / "clust"
    random.seed(7)
    torch.manual_seed(7)
    try:
        S.main([CKPT, str(clust), DB, "-k", "8", "-n", "2", "--save"])
    finally:
        for name in ("Kmean", "DPMean"):
            for h in list(logging.getLogger(name).handlers):
                logging.getLogger(name).removeHandler(h)
                h.close()
    Q.main([str(clust / "checkpoint_last.pt"), DB, str(tmp_path / "quant")])
    quantized = str(tmp_path / "quant" / "quantized_outputs.txt")
    common = ["--path_audio_data", DB, "--path_abx_item", DB_ITEM, "--file-extension", ".flac"]

    random.seed(11)
    EC.main(["--quantized", quantized, "--name-output", str(tmp_path / "scores_q.json")] + common)
    random.seed(11)
    EC.main(["--clustering", str(clust / "checkpoint_last.pt"), "--name-output", str(tmp_path / "scores_c.json")] + common)
    for name in ("scores_q.json", "scores_c.json"):
        scores = json.load(open(tmp_path / name))
        assert set(scores) == {"within", "across", "args"}
        assert 0.0 <= scores["within"] <= 1.0 and 0.0 <= scores["across"] <= 1.0
        assert scores["args"] == {"modes": ["within", "across"], "feature_size": 0.01, "distance_mode": "cosine",
                                  "path_data": DB, "file_extension": ".flac", "debug": False}
    with pytest.raises(SystemExit):                            # an existing output file is refused
        EC.main(["--quantized", quantized, "--name-output", str(tmp_path / "scores_q.json")] + common)

    # the unit path against eval_ABX.ABX on the one-hot features of the same file: same seed, same file order
    qc = EC.QuantizedClustering(quantized)
    seqs = sorted((p.stem, str(p)) for p in Path(DB).glob("**/*.flac"))
    random.seed(5)
    units = EC.eval_ABX_Librispeech(DB, DB_ITEM, qc.feature_function, modes="all", unit_function=qc.unit_function,
                                    n_units=qc.n_units, seq_list=seqs)
    random.seed(5)
    dense = eval_ABX.ABX(qc.feature_function, DB_ITEM, seqs, "cosine", 100.0, ["within", "across"], cuda=False,
                         max_x_across=5, max_size_group=10, normalize=True)
    print("end to end:", units, dense)
    assert units == dense
