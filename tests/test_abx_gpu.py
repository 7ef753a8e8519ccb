"""ABX kernels on the MI355X (cpc_abx_dtw, cpc_abx_counts) against the fp64 oracle (tests/abx_oracle.py) and the
reference's outputs in g19_abx.npz; the batched scorer against the per-group path; the command line end to end on the
committed audio."""
import json
import os
import random

import numpy as np
import pytest
import torch

from cpc2_amd.eval import eval_ABX
from cpc2_amd.eval.ABX import abx_group_computation as abx_g
from cpc2_amd.eval.ABX import abx_iterators as abx_it
from tests import abx_oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = torch.device("cuda:0")
COS, EUC = abx_g.get_cosine_distance_batch, abx_g.get_euclidian_distance_batch


@pytest.fixture(scope="module")
def g19():
    return np.load(os.path.join(GOLDEN, "g19_abx.npz"), allow_pickle=False)


def _padded(items):
    S = max(v.shape[0] for v in items)
    out = torch.zeros(len(items), S, items[0].shape[1])
    for i, v in enumerate(items):
        out[i, :v.shape[0]] = torch.from_numpy(np.asarray(v, dtype=np.float32))
    return out.to(DEV), torch.tensor([v.shape[0] for v in items])


def _normalised(rng, n, D, zero_p=0.0):
    v = torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32))
    v[torch.from_numpy(rng.random(n) < zero_p)] = 0.0
    return abx_it.normalize_with_singularity(v).numpy()


def _kernel_pairs(xs, ys, dist):
    """DTW value and path length of every (x, y) through cpc_abx_dtw."""
    a, sa = _padded(xs)
    b, sb = _padded(ys)
    items = abx_g._Items.from_padded([(a, sa), (b, sb)], DEV)
    px = np.repeat(np.arange(len(xs)), len(ys))
    py = np.tile(np.arange(len(ys)), len(xs)) + len(xs)
    vals, plen = abx_g._dtw_pairs(items, px, py, abx_g.COSINE if dist == "cosine" else abx_g.EUCLIDIAN)
    return vals.cpu().numpy().reshape(len(xs), len(ys)), plen.cpu().numpy().reshape(len(xs), len(ys))


@pytest.mark.parametrize("D", [3, 256, 512])
@pytest.mark.parametrize("dist", ["cosine", "euclidian"])
def test_dtw_kernel_matches_oracle(D, dist):
    rng = np.random.default_rng(D + (0 if dist == "cosine" else 1))
    lens = [1, 63, 64, 65, 90, 7]
    if dist == "cosine":
        xs = [_normalised(rng, n, D, 0.1) for n in lens]
        ys = [_normalised(rng, n, D, 0.1) for n in [1, 2, 64, 65, 90, 33]]
    else:
        xs = [rng.standard_normal((n, D)).astype(np.float32) for n in lens]
        ys = [rng.standard_normal((n, D)).astype(np.float32) for n in [1, 2, 64, 65, 90, 33]]
    vals, plen = _kernel_pairs(xs, ys, dist)
    for i, x in enumerate(xs):
        for j, y in enumerate(ys):
            v, n = O.dtw_items(x, y, dist)
            assert abs(vals[i, j] - v) < 1e-5 * max(1.0, abs(v)), (i, j, vals[i, j], v)
            assert plen[i, j] == n, (i, j, plen[i, j], n)          # continuous random inputs: no cost ties


def test_dtw_kernel_near_identical_frames():
    """y = x + 1e-4 noise: dot products within ~1e-7 of 1, where acos has slope 1/sqrt(1 - d^2).  An f32 dot carries
    an error of a few ulps of 1 (~6e-8 each); acos(1 - e) ~ sqrt(2 e), so 4 ulps move a distance by up to
    sqrt(2 * 2.4e-7) / pi ~ 2.2e-4: the bound is 3e-4."""
    rng = np.random.default_rng(7)
    xs, ys = [], []
    for n in (5, 17, 40):
        base = rng.standard_normal((n, 256)).astype(np.float32)
        xs.append(abx_it.normalize_with_singularity(torch.from_numpy(base.copy())).numpy())
        noisy = base + 1e-4 * rng.standard_normal((n, 256)).astype(np.float32)
        ys.append(abx_it.normalize_with_singularity(torch.from_numpy(noisy)).numpy())
    vals, _ = _kernel_pairs(xs, ys, "cosine")
    for i in range(3):
        for j in range(3):
            v, _ = O.dtw_items(xs[i], ys[j], "cosine")
            assert abs(vals[i, j] - v) < 3e-4, (i, j, vals[i, j], v)


def test_dtw_kernel_zero_frames():
    z = abx_it.normalize_with_singularity(torch.zeros(1, 8)).numpy()
    nz = abx_it.normalize_with_singularity(torch.arange(1.0, 9.0).view(1, 8)).numpy()
    vals, plen = _kernel_pairs([z, nz], [z, nz], "cosine")
    assert vals[0, 0] == 0.0 and vals[1, 1] < 1e-3 and vals[0, 1] == 1.0 and vals[1, 0] == 1.0
    assert (plen == 1).all()


def test_reference_dtw_cases_and_known_answers(g19):
    for k in range(int(g19["dtw_n"])):
        code, sym = (int(v) for v in g19[f"dtw{k}_cfg"])
        a, b = torch.from_numpy(g19[f"dtw{k}_a"]).to(DEV), torch.from_numpy(g19[f"dtw{k}_b"]).to(DEV)
        sa, sb = torch.from_numpy(g19[f"dtw{k}_sa"]), torch.from_numpy(g19[f"dtw{k}_sb"])
        out = abx_g.get_distance_group_dtw(a, b, sa, sb, ignore_diag=bool(sym), symmetric=bool(sym),
                                           distance_function=COS if code == 0 else EUC).numpy()
        ref = g19[f"dtw{k}_out"]
        is_int = np.all(g19[f"dtw{k}_a"] == np.round(g19[f"dtw{k}_a"])) and code == 1
        if is_int:
            assert np.array_equal(out, ref), k                        # exact sqrt of exact sums: tied costs, same lengths
        else:
            assert np.abs(out - ref).max() < 2e-4, (k, np.abs(out - ref).max())
    X, Y = torch.from_numpy(g19["known_X"]).to(DEV), torch.from_numpy(g19["known_Y"]).to(DEV)
    Xs, Ys = torch.from_numpy(g19["known_X_size"]), torch.from_numpy(g19["known_Y_size"])
    dist = abx_g.get_distance_group_dtw(X, Y, Xs, Ys, distance_function=EUC).numpy()
    assert np.array_equal(dist, g19["known_dist"])
    assert np.abs(dist[:, 0] - g19["known_expected"]).max() < 1e-6
    assert abx_g.get_theta_group_dtw(X, Y, X, Xs, Ys, Xs, EUC, True) == float(g19["known_theta"]) == 0.5


def _dataset(g, tag):
    prefix = f"{tag}_feat_"
    feats = {k[len(prefix):]: torch.from_numpy(g[k].copy()) for k in g.files if k.startswith(prefix)}
    return abx_it.ABXFeatureLoader(os.path.join(GOLDEN, "g19_abx_synth.item"), [(f, f) for f in sorted(feats)],
                                   lambda p: feats[p].clone(), 100.0, True)


def _oracle_bands(ds, it, trips, tol=1e-4):
    frames = [ds[i][0].numpy() for i in range(len(ds))]
    lo, hi = [], []
    for a, b, x in trips:
        dxb = O.group_dtw([frames[i] for i in x], [frames[i] for i in b], "cosine")
        dxa = O.group_dtw([frames[i] for i in x], [frames[i] for i in a], "cosine", symmetric=it.symmetric)
        n_pos = len(a) * (len(a) - 1) if it.symmetric else len(a) * len(x)
        t_lo, t_hi = O.theta_band(dxa, dxb, n_pos * len(b), tol)
        lo.append(t_lo)
        hi.append(t_hi)
    return np.array(lo), np.array(hi)


@pytest.mark.parametrize("tag", ["abx2d", "abx3d"])
def test_batched_scores_within_oracle_band_and_reference_scores(g19, tag):
    seed, _step, msg, mxa = (int(v) for v in g19[f"{tag}_cfg"])
    ds = _dataset(g19, tag)
    random.seed(seed)
    scores = []
    for mode in ("within", "across"):
        it = ds.get_iterator(mode, msg, mxa)
        sp = abx_g.get_abx_scores_dtw_on_group(it, COS, it.symmetric)
        assert np.array_equal(sp._indices().numpy().T, g19[f"{tag}_{mode}_coords"])
        scores.append(eval_ABX.score_within(sp) if mode == "within" else eval_ABX.score_across(sp))
        theta = 1 - sp._values().numpy().astype(np.float64)
        state = random.getstate()
        random.seed(seed)                                     # replay the same draws for the oracle's plan
        it2 = ds.get_iterator("within", msg, mxa)
        plan = abx_g.plan_triplets(it2)[1]
        if mode == "across":
            it2 = ds.get_iterator("across", msg, mxa)
            plan = abx_g.plan_triplets(it2)[1]
        random.setstate(state)
        lo, hi = _oracle_bands(ds, it, plan)
        assert np.all(theta >= lo - 1e-6) and np.all(theta <= hi + 1e-6), mode
    assert np.abs(np.array(scores) - g19[f"{tag}_scores"]).max() < 1e-4


@pytest.mark.parametrize("mode", ["within", "across"])
def test_batched_equals_per_group(g19, mode):
    seed, _step, msg, mxa = (int(v) for v in g19["abx2d_cfg"])
    ds = _dataset(g19, "abx2d")
    ds.cuda()
    random.seed(seed)
    it = ds.get_iterator(mode, msg, mxa)
    stats = {}
    batched = abx_g.get_abx_scores_dtw_on_group(it, COS, it.symmetric, max_pairs=60, stats=stats)
    assert stats["chunks"] > 3
    random.seed(seed)
    it = ds.get_iterator(mode, msg, mxa)
    coords, values = [], []
    for group in it:                                              # the reference's loop: one loc_dtw per triplet
        c, v = abx_g.loc_dtw(group, COS, it.symmetric)
        coords.append(c)
        values.append(v)
    assert np.array_equal(batched._indices().numpy().T, np.array(coords))
    assert np.array_equal(batched._values().numpy(), torch.FloatTensor(values).numpy())


def test_end_to_end_cli_on_committed_audio(tmp_path):
    from cpc2_amd.feature_loader import FeatureModule, buildFeature, loadModel
    ckpt = os.path.join(GOLDEN, "ref_checkpoint", "checkpoint_7.pt")
    items = os.path.join(GOLDEN, "g19_abx_test_db.item")
    db = os.path.join(GOLDEN, "test_db")
    random.seed(2024)
    eval_ABX.main(["from_checkpoint", ckpt, items, db, "--file_extension", ".flac", "--out", str(tmp_path)])
    scores = json.load(open(tmp_path / "ABX_scores.json"))
    args = json.load(open(tmp_path / "ABX_args.json"))
    assert set(scores) == {"within", "across"} and args["path_item_file"] == items
    # the oracle on the features the package's buildFeature gives, same draws
    model = loadModel([ckpt])[0]
    model.gAR.keepHidden = True
    fm = FeatureModule(model, False).cuda().eval()
    from cpc2_amd.dataset import findAllSeqs
    from pathlib import Path
    seqs = [(Path(x).stem, os.path.join(db, x)) for _, x in findAllSeqs(db, extension=".flac")[0]]
    ds = abx_it.ABXFeatureLoader(items, seqs, lambda p: buildFeature(fm, p), 100.0, True)
    random.seed(2024)
    for mode, score_fn in (("within", eval_ABX.score_within), ("across", eval_ABX.score_across)):
        it = ds.get_iterator(mode, 20, 5)
        coords, trips = abx_g.plan_triplets(it)
        lo, hi = _oracle_bands(ds, it, trips)
        board = it.get_board_size()
        bound = [score_fn(torch.sparse_coo_tensor(torch.LongTensor(coords).t(), torch.from_numpy((1 - t).astype(np.float32)),
                                                  board)) for t in (hi, lo)]
        assert bound[0] - 1e-5 <= scores[mode] <= bound[1] + 1e-5, (mode, scores[mode], bound)
        assert 0.0 <= scores[mode] < 0.6
