"""CPU checks of the clustering package (cpc2_amd.clustering): the fp64 oracle replays the reference's recorded k-means,
DP-means and KMean trajectories (golden g20), the checkpoint helpers keep the reference's layout, both command lines
parse to the reference's namespaces, the quantized line format and --split arithmetic match the reference's output
file byte for byte, the unsupported options are refused, and CPU tensors are refused."""
import json
import os
import re

import numpy as np
import pytest
import torch

import kmeans_oracle as KO
from cpc2_amd.clustering import clustering as C
from cpc2_amd.clustering import clustering_quantization as Q
from cpc2_amd.clustering import clustering_script as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KMEAN_CASES = ["km_init", "km_pis_lo", "km_pis_hi", "km_group2", "km_start_empty", "km_converge"]


@pytest.fixture(scope="module")
def g20():
    g = np.load(os.path.join(GOLDEN, "g20_kmeans.npz"), allow_pickle=False)
    return g, json.loads(str(g["meta"]))


def replay_kmean(g, m, tag):
    """kMeanGPU (clustering.py:90-205) in fp64: [(centroids, last_diff, counts) per iteration], returned centroids."""
    feats = g[f"{tag}_feats"]
    k, n_group = m["k"], m["n_group"]
    if m["start"]:
        ck = g[f"{tag}_start"].reshape(k, -1).astype(np.float64)
    else:
        torch.manual_seed(m["seed"])
        rows = []
        for i, f in enumerate(feats):
            rows.append(f.reshape(-1, f.shape[-1] // n_group))
            if i > k:
                break
        rows = np.concatenate(rows)
        ck = rows[torch.randperm(len(rows))[:k].numpy()].astype(np.float64)
    D = ck.shape[1]
    per_iter = m["perIterSize"] if m["perIterSize"] >= 0 else len(feats)
    it, stored, traj = 0, 0, []
    while it < m["MAX_ITER"]:
        sums, counts = np.zeros((k, D)), np.zeros(k, np.int64)
        for f in feats:
            x = f.reshape(-1, D)
            index, _, margin = KO.assign(x, ck)
            assert margin.min() >= 1e-3
            s, c = KO.sums_counts(x, index, k)
            sums, counts = sums + s, counts + c
            stored += 1
            if stored >= per_iter:
                break
        if stored < per_iter:
            continue
        stored, it = 0, it + 1
        new, last_diff = KO.kmeans_update(ck, sums, counts)
        traj.append((new, last_diff, counts))
        if last_diff < m["EPSILON"]:
            break
        ck = new
    return traj, ck


def _close(a, b, scale):
    return np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() <= 1e-5 * max(1.0, scale)


def _norm_log(lines):
    out = []
    for ln in lines:
        ln = re.sub(r"done in [0-9.]+ seconds", "done in T seconds", ln)
        ln = re.sub(r"Saving last checkpoint to .*/(checkpoint_\d+\.pt)", r"Saving last checkpoint to \1", ln)
        out.append(ln)
    return out


@pytest.mark.parametrize("tag", KMEAN_CASES)
def test_oracle_reproduces_kmeans_trajectory(g20, tag):
    g, meta = g20
    m = meta[tag]
    traj, ret = replay_kmean(g, m, tag)
    iters = [ln for ln in m["logs"] if ln.startswith("ITER ")]
    assert len(iters) == len(traj)
    for i, (ln, (ck, last_diff, counts)) in enumerate(zip(iters, traj), 1):
        assert f"nItems: {int(counts.sum())}." in ln
        rec = float(ln.rsplit(" ", 1)[1])
        assert _close(last_diff, rec, abs(rec)), (i, last_diff, rec)
        key = f"checkpoint_{i}"
        if key in m["checkpoints"]:
            assert _close(ck, g[f"{tag}_{key}_Ck"].reshape(ck.shape), np.abs(ck).max())
    assert _close(ret, g[f"{tag}_return"].reshape(ret.shape), np.abs(ret).max())


def test_recorded_quirks(g20):
    _, meta = g20
    conv = meta["km_converge"]
    # converged at iteration 2: the log says so, then always "ended in MAX_ITER"; the return is checkpoint_1's centroids
    assert "Clustering ended in 2 iterations out of 20" in conv["logs"]
    assert conv["logs"][-3:-1] == ["Clustering ended in 20 iterations out of 20", "Last diff 0.0"]
    assert conv["files"] == ["checkpoint_1.pt", "checkpoint_2.pt", "training_logs.txt"]
    assert meta["km_start_empty"]["logs"][-1] == "1 empty clusters out of 4"
    assert not any("empty clusters" in ln for ln in meta["km_init"]["logs"])
    # perIterSize above the loader length: the loop is re-entered, sums zeroed, `stored` kept: 7 batches, 5 + 2
    assert [ln.split(". ")[1] for ln in meta["km_pis_hi"]["logs"] if ln.startswith("ITER")][0] == "nItems: 64"


def test_kmeans_goldens_return_previous_centroids_on_convergence(g20):
    g, _ = g20
    assert np.array_equal(g["km_converge_return"], g["km_converge_checkpoint_1_Ck"])


def test_oracle_reproduces_dpmeans(g20):
    g, meta = g20
    m = meta["dp"]
    feats = g["dp_feats"]
    mu = sum(f.astype(np.float64) for f in feats).reshape(-1, feats.shape[-1]).mean(axis=0, keepdims=True) / 100
    lines = [ln for ln in m["logs"] if ln.startswith("ITER ")]
    for i in range(1, len(lines) + 1):
        sums, counts = np.zeros_like(mu), np.zeros(len(mu), np.int64)
        for f in feats:
            x = f.reshape(-1, f.shape[-1])
            index, mu, added = KO.dpmeans_batch(x, mu, m["l"])
            if added:
                sums, counts = np.concatenate([sums, np.zeros((1, mu.shape[1]))]), np.concatenate([counts, [0]])
            s, c = KO.sums_counts(x, index, len(mu))
            sums, counts = sums + s, counts + c
        new = sums / (counts[:, None] + 1e-4)
        last_diff = np.sqrt(((mu - new) ** 2).sum(1)).max()
        mu = new
        rec = float(lines[i - 1].rsplit(" ", 1)[1])
        assert _close(last_diff, rec, rec)
        assert f"mu shape: torch.Size([1, {len(mu)}, {mu.shape[1]}])" in lines[i - 1]
        if f"checkpoint_{i}" in m["checkpoints"]:
            assert _close(mu, g[f"dp_checkpoint_{i}_Ck"].reshape(mu.shape), np.abs(mu).max())
    assert _close(mu, g["dp_return"].reshape(mu.shape), np.abs(mu).max())


def test_oracle_reproduces_plain_kmean(g20):
    g, meta = g20
    m = meta["kmean"]
    X = g["kmean_C"]
    torch.manual_seed(m["seed"])
    ck = X[torch.randperm(len(X))[:m["k"]].numpy()].astype(np.float64)
    for _ in range(m["MAX_ITER"]):
        index, _, _ = KO.assign(X, ck)
        s, c = KO.sums_counts(X, index, m["k"])
        new = s / c[:, None]
        if np.sqrt(((ck - new) ** 2).sum(1)).max() < 1e-4:
            break
        ck = new
    assert _close(ck, g["kmean_return"].reshape(ck.shape), np.abs(ck).max())


def test_checkpoint_helpers_layout(tmp_path):
    ck = torch.arange(24, dtype=torch.float32).view(1, 3, 8)
    C.save_cluster_step(ck, tmp_path / "checkpoint_3.pt", mode="kMean", iter=3, last_diff=0.5)
    st = torch.load(tmp_path / "checkpoint_3.pt")
    assert set(st) == {"state_dict", "n_clusters", "dim", "iteration", "last_diff", "mode"}
    assert (st["n_clusters"], st["dim"], st["iteration"], st["last_diff"], st["mode"]) == (3, 8, 3, 0.5, "kMean")
    assert torch.equal(st["state_dict"]["Ck"], ck)
    C.save_cluster_step(ck, tmp_path / "checkpoint_last.pt")
    for name in ("checkpoint_12.pt", "checkpoint_2.pt", "checkpoint_x1.pt", "checkpoint_.pt"):
        C.save_cluster_step(ck, tmp_path / name)
    assert C.get_last_checkpoint(tmp_path).name == "checkpoint_12.pt"
    with pytest.raises(RuntimeError, match="No checkpoint found"):
        C.get_last_checkpoint(tmp_path / "nothing")
    # the cluster module loads a checkpoint to the host first
    st = torch.load(tmp_path / "checkpoint_last.pt", map_location="cpu")
    assert st["mode"] is None and st["iteration"] is None


def test_command_lines_parse_to_the_reference_defaults(g20):
    _, meta = g20
    d = meta["defaults"]
    assert vars(S.parseArgs(["ckpt.pt", "out", "db"])) == d["clustering_script"]
    assert vars(Q.parseArgs(["ckpt.pt", "db", "out"])) == d["clustering_quantization"]
    strict_false = vars(Q.parseArgs(["ckpt.pt", "db", "out", "--strict", "False"]))
    assert strict_false == d["quantization_strict_false"] and strict_false["strict"] is True


def test_quantized_lines_and_splits_match_the_reference(g20):
    g, meta = g20
    q = meta["quantization"]
    ck = g["q_Ck"]
    d = ck.shape[-1]
    lines = []
    for _, path in q["seqNames"]:
        f = g[f"q_feat_{os.path.splitext(os.path.basename(path))[0]}"]
        index, _, margin = KO.assign(f.reshape(-1, d), ck)
        assert margin.min() >= 1e-3
        lines.append(Q.quant_line(index.tolist(), f.shape[-1] // d))
    with open(os.path.join(GOLDEN, "g20_quantized_outputs.txt"), "rb") as fh:
        committed = fh.read().decode()
    assert Q.format_output(q["seqNames"], lines) == committed == q["splits"]["all"]
    assert not committed.endswith("\n")
    n = len(q["seqNames"])
    for split in ("2-3", "3-3"):
        i, s = (int(v) for v in split.split("-"))
        a, b = Q.split_bounds(n, i, s)
        assert Q.format_output(q["seqNames"][a:b], lines[a:b]) == q["splits"][split]


def test_unsupported_options_are_refused(tmp_path):
    for extra in (["--dimReduction", "x.pt"], ["--getDistanceEstimation"]):
        with pytest.raises(SystemExit, match="not supported"):
            S.main([str(tmp_path / "ckpt.pt"), str(tmp_path / "out"), str(tmp_path / "db")] + extra)
        assert not (tmp_path / "out").exists()
    with pytest.raises(SystemExit, match="not supported"):
        Q.main([str(tmp_path / "ckpt.pt"), str(tmp_path / "db"), str(tmp_path / "q"), "--separate-speaker"])
    assert not (tmp_path / "q").exists()
    with pytest.raises(NotImplementedError):
        C.distanceEstimation(None, None)


def test_cpu_tensors_are_refused():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        C.kmeans_assign(torch.randn(5, 4), torch.randn(2, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        C.kMeanCluster(torch.randn(1, 2, 4)).assign(torch.randn(1, 5, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        C.KMean(torch.randn(20, 4), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        C.kmeans_accumulate(torch.randn(5, 4), torch.zeros(5, dtype=torch.int32), torch.zeros(2, 4),
                            torch.zeros(2, dtype=torch.long))
