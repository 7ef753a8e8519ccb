"""ABX evaluation without a GPU: item files, features, grouping, the triplet planner's random draws and order, the
host-side theta / score arithmetic and the fp64 oracle, all against the reference's outputs in g19_abx.npz
(tools/make_golden_abx.py)."""
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

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ITEMS = os.path.join(GOLDEN, "g19_abx_synth.item")
TAGS = ["abx2d", "abx3d"]


@pytest.fixture(scope="module")
def g19():
    return np.load(os.path.join(GOLDEN, "g19_abx.npz"), allow_pickle=False)


def _features(g, tag):
    prefix = f"{tag}_feat_"
    return {k[len(prefix):]: torch.from_numpy(g[k].copy()) for k in g.files if k.startswith(prefix)}


def _dataset(g, tag):
    feats = _features(g, tag)
    return abx_it.ABXFeatureLoader(ITEMS, [(f, f) for f in sorted(feats)], lambda p: feats[p].clone(),
                                   float(g[f"{tag}_cfg"][1]), True)


def _plan(g, tag, record=None):
    seed, _step, msg, mxa = (int(v) for v in g[f"{tag}_cfg"])
    random.seed(seed)
    ds = _dataset(g, tag)
    out = {}
    for mode in ("within", "across"):
        it = ds.get_iterator(mode, msg, mxa)
        out[mode] = (it, abx_g.plan_triplets(it))
    return ds, out


def test_item_file_ids_in_first_seen_order():
    files, context, phone, speaker = abx_it.load_item_file(ITEMS)
    lines = open(ITEMS).read().split("\n")[1:]
    first = [ln.split() for ln in lines if ln.strip()][0]
    assert phone[first[3]] == 0 and speaker[first[6]] == 0 and context[f"{first[4]}+{first[5]}"] == 0
    assert list(files) == [f"f{i}" for i in range(6)]
    assert sum(len(v) for v in files.values()) == len([ln for ln in lines if ln.strip()])


@pytest.mark.parametrize("tag", TAGS)
def test_features_slicing_and_normalisation_match_reference(g19, tag):
    ds = _dataset(g19, tag)
    assert np.array_equal(np.array(ds.features, dtype=np.float64), g19[f"{tag}_features"])
    assert np.array_equal(ds.data.numpy(), g19[f"{tag}_data"])          # bit-identical normalised frames


def test_normalize_with_singularity_branches():
    x2 = torch.tensor([[3.0, 4.0], [0.0, 0.0]])
    y2 = abx_it.normalize_with_singularity(x2.clone())
    assert torch.allclose(y2[0], torch.tensor([0.6, 0.8, 1e-12]))
    assert torch.allclose(y2[1, :2], torch.full((2,), 2 ** -0.5)) and y2[1, 2] == -2e12
    y3 = abx_it.normalize_with_singularity(x2.clone().view(1, 2, 2))
    assert y3.shape == (1, 2, 3)
    assert torch.equal(y3[0, 1], torch.tensor([0.0, 0.0, 1e-12]))     # +1e-12 on the norm: no zero frame in 3-D


@pytest.mark.parametrize("tag", TAGS)
def test_planner_reproduces_reference_draws_and_triplet_order(g19, tag, monkeypatch):
    draws = []
    real = random.sample

    def rec(population, k):
        out = real(population, k=k)
        draws.append(json.dumps([list(v) if isinstance(v, tuple) else v for v in out]))
        return out

    monkeypatch.setattr(random, "sample", rec)
    _ds, plans = _plan(g19, tag)
    assert draws == list(g19[f"{tag}_draws"])
    for mode in ("within", "across"):
        it, (coords, trips) = plans[mode]
        assert np.array_equal(np.array(coords, dtype=np.int64), g19[f"{tag}_{mode}_coords"])
        assert len(it) == int(g19[f"{tag}_{mode}_len"])
        assert tuple(it.get_board_size()) == tuple(g19[f"{tag}_{mode}_board"])


@pytest.mark.parametrize("tag", TAGS)
def test_oracle_triplet_values_and_scores_match_reference(g19, tag):
    ds, plans = _plan(g19, tag)
    frames = [ds[i][0].numpy() for i in range(len(ds))]
    scores = []
    for mode in ("within", "across"):
        it, (coords, trips) = plans[mode]
        lt, eq, na, nb, nx, gaps = [], [], [], [], [], []
        for a, b, x in trips:
            dxb = O.group_dtw([frames[i] for i in x], [frames[i] for i in b], "cosine")
            dxa = O.group_dtw([frames[i] for i in x], [frames[i] for i in a], "cosine", symmetric=it.symmetric)
            c = O.counts(dxa, dxb)
            lt.append(c[0])
            eq.append(c[1])
            gaps.append(c[2])
            na.append(len(a))
            nb.append(len(b))
            nx.append(len(x))
        t = lambda v: torch.tensor(v, dtype=torch.int64)  # noqa: E731
        theta = abx_g.theta_from_counts(t(lt), t(eq), t(na), t(nb), t(nx), it.symmetric)
        values = (1 - theta.to(torch.float64)).to(torch.float32).numpy()
        ref = g19[f"{tag}_{mode}_values"]
        sure = np.array(gaps) > 1e-4
        assert sure.mean() > 0.9
        assert np.array_equal(values[sure], ref[sure])                  # equal counts -> bit-equal values
        assert np.abs(values - ref).max() < 0.05
        sp = torch.sparse_coo_tensor(torch.LongTensor(coords).t(), torch.from_numpy(values), it.get_board_size())
        scores.append(eval_ABX.score_within(sp) if mode == "within" else eval_ABX.score_across(sp))
    assert np.allclose(scores, g19[f"{tag}_scores"], atol=1e-4, rtol=0)


@pytest.mark.parametrize("tag", TAGS)
def test_score_aggregation_is_bit_equal_on_reference_values(g19, tag):
    out = []
    for mode, fn in (("within", eval_ABX.score_within), ("across", eval_ABX.score_across)):
        sp = torch.sparse_coo_tensor(torch.from_numpy(g19[f"{tag}_{mode}_coords"].T.copy()),
                                     torch.from_numpy(g19[f"{tag}_{mode}_values"]), tuple(g19[f"{tag}_{mode}_board"]))
        out.append(fn(sp))
    assert out == list(g19[f"{tag}_scores"])


def test_theta_arithmetic_matches_reference_scalar_ops():
    rng = np.random.default_rng(5)
    for _ in range(300):
        na, nb, nx = (int(v) for v in rng.integers(2, 31, 3))
        sym = bool(rng.integers(0, 2))
        n = (na * (na - 1) if sym else na * nx) * nb
        lt = int(rng.integers(0, n + 1))
        eq = int(rng.integers(0, n - lt + 1))
        ref = (torch.tensor(lt) + 0.5 * torch.tensor(eq))                # abx_group_computation.py:92-93, 0-dim
        ref /= n
        got = abx_g.theta_from_counts(torch.tensor([lt]), torch.tensor([eq]), torch.tensor([na]), torch.tensor([nb]),
                                      torch.tensor([nx]), sym)
        assert got.dtype == torch.float32 and got[0].item() == ref.item()


def test_oracle_matches_reference_dtw_cases(g19):
    for k in range(int(g19["dtw_n"])):
        code, sym = (int(v) for v in g19[f"dtw{k}_cfg"])
        a, sa, b, sb = (g19[f"dtw{k}_{n}"] for n in ("a", "sa", "b", "sb"))
        ref = g19[f"dtw{k}_out"]
        dist = "cosine" if code == 0 else "euclidian"
        for i in range(a.shape[0]):
            for j in range(b.shape[0]):
                if sym and i == j:
                    continue
                ii, jj = (i, j) if not sym or j > i else (j, i)
                v, _ = O.dtw_items(a[ii, :sa[ii]], b[jj, :sb[jj]], dist)
                tol = 1e-6 if code else 2e-4                              # f32 acos of the reference near dot = 1
                assert abs(v - ref[i, j]) < tol * max(1.0, abs(v)), (k, i, j, v, ref[i, j])


def test_dtw_margin_agrees_with_dtw_and_sees_ties(g19):
    n_paths = 0
    for k in range(int(g19["dtw_n"])):
        code, _sym = (int(v) for v in g19[f"dtw{k}_cfg"])
        a, sa, b, sb = (g19[f"dtw{k}_{n}"] for n in ("a", "sa", "b", "sb"))
        for i in range(a.shape[0]):
            for j in range(b.shape[0]):
                d = O.frame_distances(a[i, :sa[i]], b[j, :sb[j]], "cosine" if code == 0 else "euclidian")
                v, n, margin = O.dtw_margin(d)
                assert (v, n) == O.dtw(d)
                assert margin >= 0 and (margin < np.inf) == (min(d.shape) > 1)
                n_paths += 1
    assert n_paths > 10
    # hand-made: up = left = 1 behind the last cell, diag = 0: margin (1 - 0) / 1 there and nowhere else
    assert O.dtw_margin(np.array([[0.0, 1.0], [1.0, 0.0]])) == (0.0, 2, 1.0)
    # the tie: up = left = diag = 1 behind the last cell; diag wins, as in dtw
    tie = np.array([[1.0, 0.0], [0.0, 5.0]])
    assert O.dtw_margin(tie) == (3.0, 2, 0.0) and O.dtw(tie) == (3.0, 2)
    # only the steps taken count: cost = [[1, 2, 4], [2, 1, 2]]; the path (1,2) (1,1) (0,0) sees (up 4, left 1, diag 2),
    # then (up 2, left 2, diag 1): margins 1/2 and 1/2, and the tie between up and left at (1,1) is not the smallest two
    off = np.array([[1.0, 1.0, 2.0], [1.0, 0.0, 1.0]])
    assert O.dtw_margin(off) == (2.0 / 3.0, 3, 0.5)
    # one row, one column: no step to choose
    assert O.dtw_margin(np.ones((1, 4))) == (1.0, 4, np.inf) and O.dtw_margin(np.ones((3, 1))) == (1.0, 3, np.inf)


def test_oracle_known_answers(g19):
    X, Xs, Y, Ys = g19["known_X"], g19["known_X_size"], g19["known_Y"], g19["known_Y_size"]
    for i in range(3):
        v, _ = O.dtw_items(X[i, :Xs[i]], Y[0, :Ys[0]], "euclidian")
        assert abs(v - g19["known_expected"][i]) < 1e-12
        assert abs(v - g19["known_dist"][i, 0]) < 1e-6
    theta, _, _ = O.triplet_theta([X[i, :Xs[i]] for i in range(3)], [Y[0, :Ys[0]]], [X[i, :Xs[i]] for i in range(3)],
                                  "euclidian", True)
    assert theta == float(g19["known_theta"]) == 0.5


def test_cli_arguments():
    a = eval_ABX.parse_args(["from_checkpoint", "ck.pt", "f.item", "db", "--file_extension", ".flac", "--mode", "within",
                             "--max_size_group", "7", "--max_x_across", "3", "--feature_size", "0.02", "--seq_norm",
                             "--strict", "--max_size_seq", "32000", "--get_encoded", "--out", "o"])
    assert (a.load, a.path_checkpoint, a.path_item_file, a.path_dataset, a.file_extension) == \
        ("from_checkpoint", "ck.pt", "f.item", "db", ".flac")
    assert (a.mode, a.max_size_group, a.max_x_across, a.feature_size) == ("within", 7, 3, 0.02)
    assert a.seq_norm and a.strict and a.get_encoded and a.max_size_seq == 32000 and a.out == "o"
    b = eval_ABX.parse_args(["from_pre_computed", "f.item", "feats", "--out", "o"])
    assert (b.file_extension, b.mode, b.max_size_group, b.max_x_across) == (".pt", "all", 20, 5)
    for bad in (["from_checkpoint", "ck.pt", "f.item", "db", "--level_gru", "2"], ["from_pre_computed", "f.item", "d"],
                ["from_checkpoint", "ck.pt", "f.item", "db", "--mode", "both"]):
        with pytest.raises(SystemExit):
            eval_ABX.parse_args(bad)


def test_errors(g19, tmp_path):
    with pytest.raises(ValueError):
        abx_g.get_distance_function_from_name("manhattan")
    ds = _dataset(g19, "abx2d")
    it = ds.get_iterator("within", 3)
    with pytest.raises(ValueError, match="distance_function"):
        abx_g.get_abx_scores_dtw_on_group(it, lambda a, b: None, True)
    with pytest.raises(ValueError):
        ds.get_iterator("sideways", 3)
    # one phone per (context, speaker): no triplet
    one = tmp_path / "one.item"
    one.write_text("#header\nf0 0.10 0.20 aa n t s1\nf0 0.30 0.40 aa n t s1\nf1 0.10 0.20 aa n t s2\n")
    feats = _features(g19, "abx2d")
    ds1 = abx_it.ABXFeatureLoader(str(one), [("f0", "f0"), ("f1", "f1")], lambda p: feats[p].clone(), 100.0, True)
    for mode in ("within", "across"):
        it1 = ds1.get_iterator(mode, 3, 2)
        with pytest.raises(ValueError, match="no triplet"):
            abx_g.get_abx_scores_dtw_on_group(it1, abx_g.get_cosine_distance_batch, it1.symmetric)
    with pytest.raises(ValueError, match="no item"):
        abx_it.ABXFeatureLoader(str(one), [("zz", "zz")], lambda p: feats["f0"].clone(), 100.0, True)
    # no CPU path
    a = torch.zeros(2, 3, 4)
    s = torch.tensor([3, 2])
    with pytest.raises(RuntimeError, match="GPU"):
        abx_g.get_distance_group_dtw(a, a, s, s)
    with pytest.raises(RuntimeError, match="GPU"):
        abx_g.get_theta_group_dtw(a, a, a, s, s, s, abx_g.get_cosine_distance_batch, True)
