"""cpc2_amd.cca without a GPU: the covariance-space solver and the data-matrix oracle against sklearn's recorded fits (golden
g28, tools/make_golden_cca.py), the model file, the command line of train_cca and its refusals, and the C entry points' limits."""
import ctypes
import os
import pickle
import re
import warnings

import numpy as np
import pytest

import cca_oracle as CO
from cpc2_amd import _lib
from cpc2_amd import dataset as ds
from cpc2_amd.cca import ATTRIBUTES, CCAModel, cca_from_moments, to_sklearn
from cpc2_amd.cca import train_cca as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TAGS = ["a", "b", "c"]
# the maker holds cca_from_moments to 1e-9 of sklearn (relative to each attribute's largest magnitude); tenfold margin for
# another BLAS's order of summation
LIMIT = 1e-8


@pytest.fixture(scope="module")
def g28():
    with np.load(os.path.join(GOLDEN, "g28_cca.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _fit(g, tag):
    X, Y = g[f"{tag}_X"], g[f"{tag}_Y"]
    return cca_from_moments(*CO.moments(X, Y), int(g[f"{tag}_n_components"]))


def test_golden_holds_the_three_problems(g28):
    assert list(g28["tags"]) == TAGS
    shapes = [(g28[f"{t}_X"].shape, g28[f"{t}_Y"].shape, int(g28[f"{t}_n_components"])) for t in TAGS]
    assert shapes == [((3000, 12), (3000, 10), 4), ((2000, 24), (2000, 16), 5), ((257, 3), (257, 1), 1)]
    assert all(g28[f"{t}_X"].dtype == np.float32 and float(g28[f"{t}_deviation"]) <= 1e-9 for t in TAGS)
    assert list(g28["c_n_iter_"]) == [1]                                # q == 1 leaves the iteration after one step


@pytest.mark.parametrize("tag", TAGS)
def test_solver_on_oracle_moments_reproduces_sklearn(g28, tag):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        model = _fit(g28, tag)
    assert list(model.n_iter_) == list(g28[f"{tag}_n_iter_"])
    dev = CO.deviation(model, g28, tag)
    print(tag, "deviation", dev)
    assert dev <= LIMIT
    assert model.n_samples_ == g28[f"{tag}_X"].shape[0]


@pytest.mark.parametrize("tag", TAGS)
def test_data_matrix_oracle_reproduces_sklearn(g28, tag):
    fit = CO.cca_fit(g28[f"{tag}_X"], g28[f"{tag}_Y"], int(g28[f"{tag}_n_components"]))
    assert list(fit["n_iter_"]) == list(g28[f"{tag}_n_iter_"])
    assert CO.deviation(fit, g28, tag) <= LIMIT


def test_too_many_components_raise_sklearns_message(g28):
    m = CO.moments(g28["a_X"], g28["a_Y"])
    with pytest.raises(ValueError, match=re.escape("`n_components` upper bound is 10. Got 11 instead. Reduce `n_components`.")):
        cca_from_moments(*m, 11)
    n, sx, sy, Sxx, Sxy, Syy = m
    with pytest.raises(ValueError, match="upper bound is 5"):
        cca_from_moments(5, sx, sy, Sxx, Sxy, Syy, 6)


def test_constant_y_stops_early_with_sklearns_warning(g28):
    X = g28["c_X"]
    Y = np.full((X.shape[0], 2), 2.5, np.float32)
    with pytest.warns(UserWarning, match="y residual is constant at iteration 0"):
        model = cca_from_moments(*CO.moments(X, Y), 2)
    assert list(model.n_iter_) == [] and not model.x_weights_.any() and not model.x_rotations_.any()
    assert np.array_equal(model._y_std, np.ones(2)) and np.array_equal(model._y_mean, np.full(2, 2.5))
    # one live y column: the second component finds the residual constant
    Y2 = np.concatenate([g28["c_Y"], np.full((X.shape[0], 1), -1.0, np.float32)], axis=1)
    with pytest.warns(UserWarning, match="y residual is constant at iteration 1"):
        model = cca_from_moments(*CO.moments(X, Y2), 2)
    assert len(model.n_iter_) == 1 and model.x_weights_[:, 0].any() and not model.x_weights_[:, 1].any()


def test_model_file_round_trip_is_bit_for_bit(g28, tmp_path):
    model = _fit(g28, "b")
    path = tmp_path / "m.npz"
    model.save(path)
    back = CCAModel.load(path)
    for name in ATTRIBUTES:
        a, b = getattr(model, name), getattr(back, name)
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    assert back.n_samples_ == model.n_samples_ == 2000
    for k, v in model.moments_.items():
        assert np.array_equal(back.moments_[k], v)
    with np.load(path, allow_pickle=False) as z:                      # plain arrays only
        assert set(ATTRIBUTES) | {"n_samples_", "sx", "sy", "Sxx", "Sxy", "Syy"} == set(z.files)


def test_sklearn_object_pickles_and_transforms_like_the_recorded_fit(g28, tmp_path):
    pytest.importorskip("sklearn")
    for tag in TAGS:
        path = tmp_path / f"{tag}.pkl"
        with open(path, "wb") as f:
            pickle.dump(to_sklearn(_fit(g28, tag)), f)
        with open(path, "rb") as f:
            cca = pickle.load(f)
        xs, ys = cca.transform(g28[f"{tag}_X"], g28[f"{tag}_Y"])
        for got, ref in ((xs, g28[f"{tag}_x_scores"]), (ys, g28[f"{tag}_y_scores"])):
            assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-8 * np.abs(ref).max()


# --------------------------------------------------------------------------- the command line
def test_parse_args_defaults_are_the_references():
    args = T.parseArgs([])
    assert vars(args) == dict(path_cp_X=None, path_cp_Y=None, path_db=None, path_output=None, n_components=100,
                              file_extension=".wav", max_size_seq=10240, batch_size=8, strict=True, debug=False, no_batch=False,
                              cpu=False)
    assert T.parseArgs(["--strict", "False"]).strict is True           # type=bool: bool("False")
    assert T.parseArgs(["--strict", ""]).strict is False
    args = T.parseArgs(["--n_components", "7", "--no_batch", "--debug", "--file_extension", ".flac"])
    assert (args.n_components, args.no_batch, args.debug, args.file_extension) == (7, True, True, ".flac")


CKPT = os.path.join(GOLDEN, "ref_checkpoint", "checkpoint_7.pt")
REFUSED = [(["--cpu"], "--cpu is not supported.*no CPU fallback"),
           (["--file_extension", ".mp3"], r"--file_extension \.mp3: there is no mp3 decoder"),
           (["--path_cp_Y", "missing/checkpoint_1.pt"], "--path_cp_Y missing/checkpoint_1.pt: not an existing .pt checkpoint"),
           (["--path_cp_X", os.path.join(GOLDEN, "ref_checkpoint", "checkpoint_args.json")], "--path_cp_X .*not an existing .pt"),
           (["--n_components", "0"], "--n_components 0")]


@pytest.mark.parametrize("flags,text", REFUSED, ids=[" ".join(r[0][:1]) for r in REFUSED])
def test_main_refuses_by_name_before_the_audio_is_listed(flags, text, monkeypatch, tmp_path):
    listed = []
    monkeypatch.setattr(ds, "findAllSeqs", lambda *a, **k: listed.append(a) or ([], []))
    out = tmp_path / "out"
    base = ["--path_cp_X", CKPT, "--path_cp_Y", CKPT, "--path_db", str(tmp_path / "db"), "--path_output", str(out)]
    with pytest.raises(SystemExit, match=text):
        T.main(base + flags)
    assert not listed and not out.exists()


# --------------------------------------------------------------------------- the C entry points
def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "cpc2_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("cpc_moments_scratch_bytes", "cpc_moments_accumulate"):
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in cpc2_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES
    assert _lib.load().cpc_version() >= 118


def test_entry_points_refuse_sizes_outside_the_limits_before_any_launch():
    lib = _lib.load()
    query = lib.cpc_moments_scratch_bytes
    assert query(1, 1, 0) > 0 and query(1 << 20, 512, 512) > 0 and query((1 << 31) - 1, 512, 512) > 0
    one = ctypes.c_void_p(256)                                          # never dereferenced: refused before any launch

    def call(dx, dy, n, ldx=None, ldy=None, y=one):
        return lib.cpc_moments_accumulate(one, dx if ldx is None else ldx, dx, y, dy if ldy is None else ldy, dy, n, one, one,
                                          one, 1 << 40, None)
    for dx, dy, n in [(0, 0, 5), (513, 0, 5), (4, 513, 5), (4, 3, 0), (4, -1, 5), (4, 3, 1 << 31)]:
        assert query(n, dx, dy) == 0
        assert call(dx, dy, n) == -1 and b"sizes outside the supported limits" in lib.cpc_last_error()
    assert call(4, 3, 5, ldx=3) == -1 and b"row stride" in lib.cpc_last_error()
    assert call(4, 3, 5, ldy=2) == -1 and b"row stride" in lib.cpc_last_error()
    assert call(4, 3, 5, y=None) == -1 and b"null buffer" in lib.cpc_last_error()
    assert lib.cpc_moments_accumulate(None, 4, 4, None, 0, 0, 5, None, None, None, 0, None) == -1
    # a scratch buffer below the query's size is refused too
    assert lib.cpc_moments_accumulate(one, 4, 4, one, 3, 3, 5, one, one, one, 16, None) == -1 and b"scratch" in lib.cpc_last_error()
