"""ABX on quantized units without a GPU: QuantizedClustering's parsing, the unit store (ABXUnitLoader) against the
reference's loader, the fp64 oracle on the one-hot expansions against the reference's per-triplet values in
g22_abx_units.npz (tools/make_golden_abx_units.py) -- exactly --, the two frame distances, the ABI and the command line."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

from cpc2_amd import _lib
from cpc2_amd.eval import eval_ABX
from cpc2_amd.eval import eval_ABX_clustering as EC
from cpc2_amd.eval.ABX import abx_group_computation as abx_g
from cpc2_amd.eval.ABX import abx_iterators as abx_it
from tests import abx_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ITEM = os.path.join(GOLDEN, "g19_abx_synth.item")
VARIANTS = {"u8": ("g22_quantized_units.txt", None), "u50": ("g22_quantized_units_50.txt", None),
            "ug": ("g22_quantized_units_groups.txt", "g22_onehot_dict.txt")}
SEQS = [(f"f{f}", f"f{f}.flac") for f in range(6)]


@pytest.fixture(scope="module")
def g22():
    return np.load(os.path.join(GOLDEN, "g22_abx_units.npz"), allow_pickle=False)


def _maker(tag):
    name, dic = VARIANTS[tag]
    return EC.QuantizedClustering(os.path.join(GOLDEN, name), os.path.join(GOLDEN, dic) if dic else None)


def _store(g, tag):
    qc = _maker(tag)
    return qc, abx_it.ABXUnitLoader(ITEM, SEQS, qc.unit_function, float(g[f"{tag}_cfg"][1]), True, qc.n_units)


# --------------------------------------------------------------------------- parsing
def test_quantized_file_integer_form(tmp_path):
    path = tmp_path / "q.txt"
    path.write_text("some/dir/a.flac\t1,2,2,7\nb\t0,5")                  # no trailing newline; a path and a bare stem
    qc = EC.QuantizedClustering(str(path))
    assert qc.n_units == 8 and qc.step_feature_multiplication == 1 and qc.has_units
    assert set(qc.frames_dict) == {"a", "b"} and qc.frames_dict["b"] == [0, 5]
    units = qc.unit_function("/elsewhere/a.wav")                          # looked up by stem
    assert units.dtype == torch.int64 and units.tolist() == [1, 2, 2, 7]
    path.write_text("a\t1,2,2,7\nb\t0,5\n")                                # a trailing newline changes nothing
    assert EC.QuantizedClustering(str(path)).frames_dict == qc.frames_dict


def test_quantized_file_dictionary_form(tmp_path):
    path = tmp_path / "q.txt"
    path.write_text("a\t3-1,3-1,0-2\nb\t0-0")
    with pytest.raises(AssertionError, match="dictionary must be given"):
        EC.QuantizedClustering(str(path))
    dic = tmp_path / "dict.txt"
    dic.write_text("0-0 12\n3-1 7\n\n0-2 1\n")                            # an empty line keeps its index
    qc = EC.QuantizedClustering(str(path), onehot_dict=str(dic))
    assert qc.frames_dict == {"a": [1, 1, 3], "b": [0]} and qc.n_units == 4
    with pytest.raises(KeyError):
        path.write_text("a\t9-9")
        EC.QuantizedClustering(str(path), onehot_dict=str(dic))


@pytest.mark.parametrize("tag", list(VARIANTS))
def test_golden_files_parse(g22, tag):
    qc = _maker(tag)
    assert qc.n_units == int(g22[f"{tag}_cfg"][4])
    assert list(qc.frames_dict) == [f"f{f}" for f in range(6)]
    assert all(len(v) == 400 for v in qc.frames_dict.values())
    assert not open(os.path.join(GOLDEN, VARIANTS[tag][0])).read().endswith("\n")


# --------------------------------------------------------------------------- the unit store
@pytest.mark.parametrize("tag", list(VARIANTS))
def test_unit_store_holds_the_reference_loaders_items(g22, tag):
    qc, ds = _store(g22, tag)
    assert np.array_equal(np.array(ds.features, dtype=np.float64), g22[f"{tag}_features"])
    assert ds.units.dtype == torch.int32 and ds.units.dim() == 1
    assert np.array_equal(ds.units.numpy(), g22[f"{tag}_data_units"])     # = argmax of the reference loader's data
    assert ds.feature_dim == qc.n_units + 1 and not hasattr(ds, "data")
    # the rows an item expands to are the reference loader's: 0, 1e-12 and 1, the 1 at the unit
    rows, size, ids = ds[3]
    off = ds.features[3][0]
    assert rows.shape == (size, qc.n_units + 1) and rows.dtype == torch.float32 and ids == tuple(ds.features[3][2:])
    assert np.array_equal(np.unique(rows.numpy()), g22[f"{tag}_data_values"])
    assert np.array_equal(rows[:, :-1].argmax(1).numpy(), ds.units[off:off + size].numpy())
    assert (rows[:, -1] == np.float32(1e-12)).all() and (rows[:, :-1].sum(1) == 1).all()
    # the same rows as the dense loader on feature_function's one-hot tensor (host side: .cuda() of the maker stubbed)
    dense = abx_it.ABXFeatureLoader(ITEM, SEQS, lambda p: EC.one_hot(qc.unit_function(p), qc.n_units).unsqueeze(0),
                                    100.0, True)
    assert dense.features == ds.features and torch.equal(dense[3][0], rows)
    it = ds.get_iterator("within", 10)
    data, sizes, _ = it.group_data([0, 3, 5])
    assert data.shape == (3, int(sizes.max()), qc.n_units + 1) and torch.equal(data[1, :size], rows)


def test_unit_store_refuses_what_is_not_a_unit():
    with pytest.raises(TypeError, match="integer unit ids"):
        abx_it.ABXUnitLoader(ITEM, SEQS, lambda p: torch.zeros(400), 100.0, True, 8)
    with pytest.raises(ValueError, match="outside"):
        abx_it.ABXUnitLoader(ITEM, SEQS, lambda p: torch.full((400,), 8), 100.0, True, 8)
    with pytest.raises(ValueError, match="no item"):
        abx_it.ABXUnitLoader(ITEM, [("nope", "nope")], lambda p: torch.zeros(400, dtype=torch.long), 100.0, True, 8)
    ds = abx_it.ABXUnitLoader(ITEM, SEQS, lambda p: torch.zeros(400, dtype=torch.long), 100.0, True, 8)
    with pytest.raises(RuntimeError, match="unit ids, not frames"):
        ds.device_frames(torch.device("cpu"), 12)


def test_frame_distances_of_one_hot_rows():
    cos, euc = abx_g.get_cosine_distance_batch, abx_g.get_euclidian_distance_batch
    for n in (1, 2, 8, 2000):
        for normalize in (True, False):
            assert abx_g.unit_frame_distances(n, normalize, cos) == (0.0, 0.5)
            assert abx_g.unit_frame_distances(n, normalize, euc) == (0.0, float(np.sqrt(np.float32(2))))
    with pytest.raises(ValueError, match="unsupported distance_function"):
        abx_g.unit_frame_distances(8, True, max)


# --------------------------------------------------------------------------- oracle against the golden, exactly
@pytest.mark.parametrize("tag", list(VARIANTS))
def test_oracle_on_one_hot_expansions_equals_reference_values(g22, tag):
    seed, _step, msg, mxa, _n = (int(v) for v in g22[f"{tag}_cfg"])
    _qc, ds = _store(g22, tag)
    frames = [ds[i][0].numpy() for i in range(len(ds))]
    cache = {}

    def dtw(i, j):
        if (i, j) not in cache:
            cache[i, j] = O.dtw_items(frames[i], frames[j], "cosine")[0]
        return cache[i, j]

    random.seed(seed)
    scores = []
    for mode in ("within", "across"):
        it = ds.get_iterator(mode, msg, mxa)
        coords, trips = abx_g.plan_triplets(it)
        assert np.array_equal(np.array(coords, dtype=np.int64), g22[f"{tag}_{mode}_coords"])
        assert tuple(it.get_board_size()) == tuple(g22[f"{tag}_{mode}_board"])
        lt, eq, na, nb, nx, gaps = [], [], [], [], [], []
        for a, b, x in trips:
            dxb = np.array([[dtw(i, k) for k in b] for i in x])
            if it.symmetric:                                  # j > i computed as (x_i, a_j) and mirrored, diagonal excluded
                dxa = np.array([[np.nan if p == q else dtw(x[min(p, q)], a[max(p, q)]) for q in range(len(a))]
                                for p in range(len(x))])
            else:
                dxa = np.array([[dtw(i, j) for j in a] for i in x])
            c = O.counts(dxa, dxb)
            lt.append(c[0])
            eq.append(c[1])
            d = np.abs(dxa[:, :, None] - dxb[:, None, :])
            gaps.append(d[d > 0].min() if (d > 0).any() else np.inf)
            na.append(len(a))
            nb.append(len(b))
            nx.append(len(x))
        t = lambda v: torch.tensor(v, dtype=torch.int64)  # noqa: E731
        theta = abx_g.theta_from_counts(t(lt), t(eq), t(na), t(nb), t(nx), it.symmetric)
        values = (1 - theta.to(torch.float64)).to(torch.float32).numpy()
        assert min(gaps) > 1e-4                               # no comparison is near a flip (every cost is a multiple of 0.5)
        assert np.array_equal(values, g22[f"{tag}_{mode}_values"]), mode
        sp = torch.sparse_coo_tensor(torch.LongTensor(coords).t(), torch.from_numpy(values), it.get_board_size())
        scores.append(eval_ABX.score_within(sp) if mode == "within" else eval_ABX.score_across(sp))
    assert np.allclose(scores, g22[f"{tag}_scores"], atol=1e-4, rtol=0)


def test_oracle_equals_reference_dtw_cases(g22):
    def expand(u, n_units):
        rows = torch.zeros(1, len(u), n_units)
        rows.scatter_(-1, torch.from_numpy(u.astype(np.int64)).view(1, -1, 1), 1)
        return abx_it.normalize_with_singularity(rows)[0].numpy()
    for k in range(int(g22["dtw_n"])):
        code, sym, n_units = (int(v) for v in g22[f"dtw{k}_cfg"])
        xs = [expand(row[row >= 0], n_units) for row in g22[f"dtw{k}_x"]]
        ys = [expand(row[row >= 0], n_units) for row in g22[f"dtw{k}_y"]]
        ref = g22[f"dtw{k}_out"]
        for i, x in enumerate(xs):
            for j, y in enumerate(ys):
                if sym and j <= i:
                    continue
                v = O.dtw_items(x, y, "cosine" if code == 0 else "euclidian")[0]
                if code == 0:
                    assert np.float32(v) == ref[i, j], (k, i, j)          # multiples of 0.5 over an integer: exact
                else:
                    assert abs(v - ref[i, j]) < 1e-5 * max(1.0, abs(v)), (k, i, j)


# --------------------------------------------------------------------------- ABI
def test_abi_declares_the_unit_kernel():
    header = open(os.path.join(ROOT, "include", "cpc2_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(cpc_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("cpc_abx_dtw_units", "cpc_abx_dtw_units_scratch_bytes"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert len(_lib.SIGNATURES["cpc_abx_dtw_units"][1]) == 17
    assert _lib.load().cpc_version() >= 110
    q = _lib.load().cpc_abx_dtw_units_scratch_bytes
    assert q(0, 10, 10) == 0 and q(5, 64, 100) == 0 and q(5, 65, 100) > 0
    assert "abx_units.hip" in open(os.path.join(ROOT, "cpc2_amd", "build.py")).read()


def test_scratch_query_is_pinned():
    """0 when one strip holds every x item; else min(n_seg, 8192) workgroups x 4 waves x 2 buffers x 8 bytes x max_len_y: the
    grid cap of the dense kernels, not the 2048 of the two term kernels on units."""
    lib = _lib.load()
    size = lib.cpc_abx_dtw_units_scratch_bytes
    for n_seg in (1, 100, 8192, 20000):
        for max_len_x in (64, 65):
            for max_len_y in (1, 500):
                want = 0 if max_len_x <= 64 else min(n_seg, 8192) * 4 * 2 * 8 * max_len_y
                assert size(n_seg, max_len_x, max_len_y) == want, (n_seg, max_len_x, max_len_y)
    assert size(0, 65, 500) == 0
    for bad in ((-1, 65, 500), (5, -65, 500), (5, 65, -500)):
        assert size(*bad) == 0
        message = lib.cpc_last_error()
        assert message.startswith(b"abx_dtw_units:") and b"negative size" in message, message


# --------------------------------------------------------------------------- command line
def test_command_line(tmp_path, capsys):
    base = ["--path_audio_data", "db", "--path_abx_item", "x.item"]
    args = EC.parse_args(["--quantized", "q.txt"] + base)
    assert args.quantized == "q.txt" and args.clustering is None and args.modes == "all" and args.feature_size == 0.01
    assert args.gru == -1 and args.file_extension == ".flac" and not args.soft_clustering and args.group_modes == "onehot"
    assert args.onehot_dict is None and not args.debug and not args.no_save and args.name_output is None
    args = EC.parse_args(["--clustering", "c.pt", "-s", "--group-modes", "seq", "--modes", "within", "--feature-size",
                          "0.02", "--gru", "2", "--no-save", "--debug", "--onehot-dict", "d.txt", "--file-extension",
                          ".wav", "--name-output", str(tmp_path / "new.json")] + base)
    assert args.clustering == "c.pt" and args.soft_clustering and args.group_modes == "seq" and args.gru == 2
    for bad in (base,                                                               # one input is required
                ["--quantized", "q", "--clustering", "c"] + base,                    # ... and only one
                ["--quantized", "q", "--path_abx_item", "x.item"],                   # no default paths
                ["--quantized", "q", "--path_audio_data", "db"],
                ["--quantized", "q", "--group-modes", "concat"] + base):
        with pytest.raises(SystemExit):
            EC.parse_args(bad)
    existing = tmp_path / "scores.json"
    existing.write_text("{}")
    with pytest.raises(SystemExit):
        EC.parse_args(["--quantized", "q", "--name-output", str(existing)] + base)
    assert "already exists" in capsys.readouterr().err
    with pytest.raises(AssertionError, match="already exists"):
        EC.eval_ABX_Librispeech("db", ITEM, None, path_output=str(existing))
    assert existing.read_text() == "{}"
    with pytest.raises(AssertionError):
        EC.eval_ABX_Librispeech("db", ITEM, None, modes="both")
    with pytest.raises(AssertionError):
        EC.eval_ABX_Librispeech("db", ITEM, None, distance_mode="manhattan")
    with pytest.raises(ValueError, match="go together"):
        EC.eval_ABX_Librispeech("db", ITEM, None, unit_function=lambda p: None)

