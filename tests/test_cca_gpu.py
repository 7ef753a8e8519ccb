"""cpc2_amd.cca on the GPU: Moments and the solve against sklearn's recorded fits (golden g28), CCAModel.transform against the
recorded sklearn transform, and python -m cpc2_amd.cca.train_cca end to end on the committed audio.  No sklearn import here."""
import argparse
import importlib.util
import json
import os
import shutil

import numpy as np
import pytest
import torch

import cca_oracle as CO
from cpc2_amd.cca import ATTRIBUTES, CCAModel, Moments, cca_from_moments

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEV = torch.device("cuda:0")
TAGS = ["a", "b", "c"]


@pytest.fixture(scope="module")
def g28():
    with np.load(os.path.join(GOLDEN, "g28_cca.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def fitted(g28):
    """tag -> (Moments.state() of the inputs fed in ragged chunks, the model fitted on it)"""
    out = {}
    for tag in TAGS:
        X, Y = torch.from_numpy(g28[f"{tag}_X"]).to(DEV), torch.from_numpy(g28[f"{tag}_Y"]).to(DEV)
        m = Moments(X.shape[1], Y.shape[1], device=DEV)
        start = 0
        for size in (1, 7, 1000, X.shape[0]):
            stop = min(X.shape[0], start + size)
            if stop > start:
                m.update(X[start:stop], Y[start:stop])
            start = stop
        state = m.state()
        out[tag] = (state, cca_from_moments(*state, int(g28[f"{tag}_n_components"])))
    return out


def _within_bound(state, X, Y):
    n, sx, sy, Sxx, Sxy, Syy = state
    rn, rsx, rsy, rSxx, rSxy, rSyy = CO.moments(X, Y)
    bs, bg = CO.moments_bound(X, Y)
    assert n == rn
    assert (np.abs(np.concatenate([sx, sy]) - np.concatenate([rsx, rsy])) <= bs).all()
    assert (np.abs(np.block([[Sxx, Sxy], [Sxy.T, Syy]]) - np.block([[rSxx, rSxy], [rSxy.T, rSyy]])) <= bg).all()


@pytest.mark.parametrize("tag", TAGS)
def test_moments_and_solve_reproduce_sklearn(g28, fitted, tag):
    state, model = fitted[tag]
    _within_bound(state, g28[f"{tag}_X"], g28[f"{tag}_Y"])
    assert list(model.n_iter_) == list(g28[f"{tag}_n_iter_"])
    dev = CO.deviation(model, g28, tag)
    print(tag, "deviation from sklearn", dev)
    assert dev <= 1e-8


@pytest.mark.parametrize("tag", TAGS)
def test_transform_against_the_recorded_sklearn_transform(g28, fitted, tag):
    """The device computes x W^T + b in f32 with the centring and scaling folded into W and b (in f64, then rounded to f32), so
    the first-order bound of its error is that of an f32 dot product over the p terms it sums, W and b rounded once each and the
    bias added:  (p + 4) 2^-24 (sum_j |W[c][j]| |x[j]| + |b[c]|)  per output, as tests/test_resample_gpu.py forms it."""
    _, model = fitted[tag]
    X, Y = g28[f"{tag}_X"], g28[f"{tag}_Y"]
    xs, ys = model.transform(torch.from_numpy(X).to(DEV), torch.from_numpy(Y).to(DEV))
    assert xs.is_cuda and xs.dtype == torch.float32
    for got, ref, data, mean, std, rot in ((xs, g28[f"{tag}_x_scores"], X, model._x_mean, model._x_std, model.x_rotations_),
                                           (ys, g28[f"{tag}_y_scores"], Y, model._y_mean, model._y_std, model.y_rotations_)):
        w = rot / std[:, None]                                           # [d, components]
        b = -(mean / std) @ rot
        scale = np.abs(data.astype(np.float64)) @ np.abs(w) + np.abs(b)
        bound = (data.shape[1] + 4) * 2.0 ** -24 * scale
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
        print(tag, "transform: worst error / bound %.3f, worst error %.3e of scores up to %.2f" %
              ((err / bound).max(), err.max(), np.abs(ref).max()))
        assert got.shape == ref.shape and (err <= bound).all()
    only_x = model.transform(torch.from_numpy(X).to(DEV).view(1, *X.shape))
    assert only_x.shape == (1, X.shape[0], model.n_components) and torch.equal(only_x[0], xs)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.transform(torch.from_numpy(X))


# --------------------------------------------------------------------------- end to end on the committed audio
def _write_run(run, seed):
    """A run directory with a seeded, untrained hidden-32 model."""
    from cpc2_amd.model import CPCModel
    from cpc2_amd.train import getAR, getEncoder
    run.mkdir()
    args = json.load(open(os.path.join(GOLDEN, "ref_checkpoint", "checkpoint_args.json")))
    json.dump(args, open(run / "checkpoint_args.json", "w"))
    shutil.copy(os.path.join(GOLDEN, "ref_checkpoint", "checkpoint_logs.json"), run / "checkpoint_logs.json")
    torch.manual_seed(seed)
    model = CPCModel(getEncoder(argparse.Namespace(**args)), getAR(argparse.Namespace(**args)))
    torch.save({"gEncoder": model.state_dict()}, run / "checkpoint_0.pt")
    return str(run / "checkpoint_0.pt")


@pytest.mark.parametrize("mode", ["batch", "no_batch"])
def test_train_cca_end_to_end(tmp_path, mode):
    from cpc2_amd.cca import train_cca as T
    from cpc2_amd.dataset import findAllSeqs
    from cpc2_amd.feature_loader import buildFeature, buildFeature_batch
    cp_x, cp_y = _write_run(tmp_path / "runX", 11), _write_run(tmp_path / "runY", 12)
    db = tmp_path / "db"                                                 # (the tool leaves its sequence cache in the data set)
    shutil.copytree(os.path.join(GOLDEN, "test_db"), db)
    out = tmp_path / "out"
    argv = ["--path_cp_X", cp_x, "--path_cp_Y", cp_y, "--path_db", str(db), "--path_output", str(out), "--n_components", "4",
            "--file_extension", ".flac"] + (["--no_batch"] if mode == "no_batch" else [])
    T.main(argv)
    want = {"CCA_info_args.json", "cca_model_n_components_4.npz"}
    if importlib.util.find_spec("sklearn") is not None:
        want.add("cca_model_n_components_4.pkl")
    assert set(os.listdir(out)) == want
    info = json.load(open(out / "CCA_info_args.json"))
    assert info["n_components"] == 4 and info["no_batch"] == (mode == "no_batch") and info["strict"] is True

    # the stored moments are those of the features the existing host-returning readers give, file by file
    no_batch = mode == "no_batch"
    fm_x, fm_y = T.loadFeatureMakerCPC(cp_x, no_batch).cuda(), T.loadFeatureMakerCPC(cp_y, no_batch).cuda()
    feats_x, feats_y = [], []
    for _, rel in findAllSeqs(str(db), speaker_level=0, extension=".flac")[0]:
        path = os.path.join(str(db), rel)
        for fm, feats in ((fm_x, feats_x), (fm_y, feats_y)):
            if no_batch:
                feats.append(buildFeature(fm, path, seqNorm=False, strict=True)[0].numpy())
            else:
                feats.append(buildFeature_batch(fm, path, seqNorm=False, strict=True, maxSizeSeq=10240, batch_size=8)[0].numpy())
    X, Y = np.concatenate(feats_x), np.concatenate(feats_y)
    assert X.shape == (Y.shape[0], 32) and Y.shape[1] == 32 and X.shape[0] > 1000
    model = CCAModel.load(out / "cca_model_n_components_4.npz")
    assert model.n_samples_ == X.shape[0]
    stored = (model.n_samples_,) + tuple(model.moments_[k] for k in ("sx", "sy", "Sxx", "Sxy", "Syy"))
    _within_bound(stored, X, Y)
    # and the stored attributes are the solve of the stored moments
    again = cca_from_moments(*stored, 4)
    for name in ATTRIBUTES:
        assert np.array_equal(getattr(model, name), getattr(again, name)), name
    assert model.x_rotations_.shape == (32, 4) and np.isfinite(model.x_rotations_).all()


def test_train_cca_refuses_too_many_components_before_extraction(tmp_path, monkeypatch):
    from cpc2_amd import feature_loader as FL
    from cpc2_amd.cca import train_cca as T
    cp = _write_run(tmp_path / "run", 3)
    db = tmp_path / "db"
    shutil.copytree(os.path.join(GOLDEN, "test_db"), db)

    def no_features(*a, **k):
        raise AssertionError("features were extracted")
    monkeypatch.setattr(FL, "buildFeature_batch_device", no_features)
    with pytest.raises(SystemExit, match="--n_components 33 is above the narrower feature width"):
        T.main(["--path_cp_X", cp, "--path_cp_Y", cp, "--path_db", str(db), "--path_output", str(tmp_path / "out"),
                "--n_components", "33", "--file_extension", ".flac"])
