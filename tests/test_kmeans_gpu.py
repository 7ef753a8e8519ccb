"""k-means kernels (csrc/kmeans.hip) and the clustering package on the GPU: assignment, distances and accumulation against
the fp64 oracle, the reference's recorded kMeanGPU / fastDPMean / KMean trajectories (golden g20), and both command
lines end to end on the committed audio."""
import argparse
import json
import os
import random
import shutil

import numpy as np
import pytest
import torch

import kmeans_oracle as KO
from cpc2_amd.clustering import clustering as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEV = torch.device("cuda:0")


def _oracle_gpu(x, ck):
    """fp64 [n, k] distances, computed on the device in chunks (direct form)."""
    x64, c64 = x.double(), ck.double()
    out = torch.empty(x.size(0), ck.size(0), dtype=torch.float64, device=x.device)
    step = max(1, (1 << 26) // max(1, ck.size(0) * ck.size(1)))
    for i in range(0, x.size(0), step):
        out[i:i + step] = ((x64[i:i + step, None, :] - c64[None]) ** 2).sum(dim=2)
    return out


def _best_two(dist):
    if dist.size(1) == 1:
        return dist[:, 0], torch.full_like(dist[:, 0], float("inf"))
    two = dist.topk(2, dim=1, largest=False).values
    return two[:, 0], two[:, 1]


# --------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("d", [1, 3, 4, 31, 32, 100, 256, 512, 1024])
def test_assign_against_oracle(d):
    gen = torch.Generator().manual_seed(d)
    for k in [1, 2, 50, 63, 64, 65, 500, 2000]:
        ck = torch.randn(k, d, generator=gen).to(DEV)
        for n in [1, 7, 1000, 32017]:
            x = torch.randn(n, d, generator=gen).to(DEV)
            index, min_sq = C.kmeans_assign(x, ck)
            ref = _oracle_gpu(x, ck)
            best, second = _best_two(ref)
            margin = (second - best) / second.abs().clamp_min(1e-30)
            ref_idx = ref.argmin(dim=1)
            clear = margin > 1e-5
            assert torch.equal(index.long()[clear], ref_idx[clear]), (n, d, k)
            # min_sq is the distance of the chosen centroid, within 1e-5 of the oracle's
            chosen = ref.gather(1, index.long().view(-1, 1)).view(-1)
            rel = ((min_sq.double() - chosen).abs() / chosen.abs().clamp_min(1e-30)).max().item()
            assert rel < 1e-5, (n, d, k, rel)
            assert ((min_sq.double() - best).abs() / best.abs().clamp_min(1e-30)).max().item() < 1e-5


def test_ties_take_the_lowest_index():
    gen = torch.Generator().manual_seed(3)
    base = torch.randint(-3, 4, (40, 7), generator=gen).float()
    ck = torch.cat([base, base, base[:5]], dim=0).to(DEV)          # every centroid duplicated at least once
    x = torch.randint(-3, 4, (5000, 7), generator=gen).float().to(DEV)
    index, min_sq = C.kmeans_assign(x, ck)
    dist = C.kmeans_distances(x, ck)
    ref = KO.sq_distances(x.cpu().numpy(), ck.cpu().numpy())          # integers: exact in f32 and fp64
    assert np.array_equal(dist.cpu().numpy(), ref.astype(np.float32))
    assert np.array_equal(index.cpu().numpy(), ref.argmin(axis=1))     # numpy: the first index of the minimum
    assert index.max().item() < 40
    # a centroid equal to every row: all distances 0, index 0 wins over identical centroids at 1..3
    z = torch.zeros(300, 129, device=DEV)
    index, min_sq = C.kmeans_assign(z, torch.zeros(4, 129, device=DEV))
    assert index.eq(0).all() and min_sq.eq(0).all()
    index, _ = C.kmeans_assign(z, torch.cat([torch.ones(200, 129), torch.zeros(3, 129)]).to(DEV))
    assert index.eq(200).all()


@pytest.mark.parametrize("n,d,k", [(1, 1, 1), (7, 3, 65), (1000, 100, 500), (4097, 256, 2000), (333, 1024, 129)])
def test_distances_against_oracle_and_assign(n, d, k):
    gen = torch.Generator().manual_seed(n + d + k)
    x = torch.randn(n, d, generator=gen).to(DEV)
    ck = torch.randn(k, d, generator=gen).to(DEV)
    dist = C.kmeans_distances(x, ck)
    ref = _oracle_gpu(x, ck)
    assert ((dist.double() - ref).abs() / ref.abs().clamp_min(1e-30)).max().item() < 1e-5
    index, min_sq = C.kmeans_assign(x, ck)
    assert torch.equal(index.long(), dist.argmin(dim=1))
    assert torch.equal(min_sq, dist.min(dim=1).values)


def _check_accumulate(x, index, k, sums0=None, counts0=None):
    d = x.size(1)
    sums = torch.zeros(k, d, device=DEV) if sums0 is None else sums0.clone()
    counts = torch.zeros(k, dtype=torch.long, device=DEV) if counts0 is None else counts0.clone()
    C.kmeans_accumulate(x, index.int(), sums, counts)
    rs, rc = KO.sums_counts(x.cpu().numpy(), index.cpu().numpy(), k)
    if sums0 is not None:
        rs = rs + sums0.cpu().double().numpy()
        rc = rc + counts0.cpu().numpy()
    assert np.array_equal(counts.cpu().numpy(), rc)
    scale, _ = KO.sums_counts(np.abs(x.cpu().numpy()), index.cpu().numpy(), k)
    if sums0 is not None:
        scale = scale + np.abs(sums0.cpu().double().numpy())
    err = np.abs(sums.cpu().double().numpy() - rs) / np.maximum(scale, 1e-30)
    assert err.max() < 1e-5, err.max()
    return sums, counts


@pytest.mark.parametrize("n,d,k", [(1, 1, 1), (1000, 3, 7), (32017, 256, 2000), (5000, 100, 50), (70000, 32, 3000)])
def test_accumulate_against_oracle(n, d, k):
    gen = torch.Generator().manual_seed(n * 7 + k)
    x = torch.randn(n, d, generator=gen).to(DEV)
    index = torch.randint(0, k, (n,), generator=gen)
    index[::5] = index[::5] % max(1, k // 10)                          # skew: a few large clusters
    _check_accumulate(x, index.to(DEV), k)
    # running accumulators: a second batch adds to the first
    s0 = torch.randn(k, d, generator=gen).to(DEV)
    c0 = torch.randint(0, 100, (k,), generator=gen).to(DEV)
    _check_accumulate(x, index.to(DEV), k, s0, c0)


def test_accumulate_empty_clusters_and_skipped_rows():
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(3000, 40, generator=gen).to(DEV)
    index = torch.randint(0, 5, (3000,), generator=gen) * 3              # clusters 1, 2, 4, 5, ... stay empty
    index[:17] = -1                                                    # out of range: skipped
    index[17:30] = 15
    s0 = torch.randn(16, 40, generator=gen).to(DEV)
    c0 = torch.arange(16).to(DEV)
    sums, counts = _check_accumulate(x, index.to(DEV), 15, s0[:15], c0[:15])
    empty = [c for c in range(15) if c % 3]
    assert torch.equal(sums[empty], s0[empty]) and torch.equal(counts[empty], c0[empty])


def test_accumulate_one_cluster_owns_every_row_and_repeats_bitwise():
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(200000, 64, generator=gen).to(DEV)
    index = torch.full((200000,), 3, dtype=torch.int32, device=DEV)
    s1, c1 = _check_accumulate(x, index, 8)
    assert c1.tolist() == [0, 0, 0, 200000, 0, 0, 0, 0]
    s2, c2 = _check_accumulate(x, index, 8)
    assert torch.equal(s1, s2) and torch.equal(c1, c2)
    mixed = torch.randint(0, 500, (200000,), generator=gen).int().to(DEV)
    a, _ = _check_accumulate(x, mixed, 500)
    b, _ = _check_accumulate(x, mixed, 500)
    assert torch.equal(a, b)


def test_limits_are_refused():
    x = torch.randn(10, 4097, device=DEV)
    with pytest.raises(ValueError, match="supported limits"):
        C.kmeans_assign(x, torch.randn(3, 4097, device=DEV))
    with pytest.raises(ValueError):
        C.kmeans_assign(torch.randn(10, 4, device=DEV), torch.randn(3, 5, device=DEV))
    index, _ = C.kmeans_assign(torch.randn(10, 4, device=DEV), torch.randn(3, 4, device=DEV))   # the next call works
    assert index.shape == (10,)


def test_cluster_step_does_not_materialise_distances():
    n, k, d = 32000, 2000, 512
    x = torch.randn(n, 1, d, device=DEV)
    step = C.kMeanClusterStep(k, d).to(DEV)
    step.Ck.copy_(torch.randn(1, k, d, device=DEV))
    step(x)                                                            # warm the scratch arena
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    Ck1, nItems = step(x)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before < n * k * 4
    assert int(nItems.sum()) == n and Ck1.shape == (1, k, d)
    # against the fp64 oracle, where the assignment is clear
    index, _, margin = KO.assign(x[:2000, 0].cpu().numpy(), step.Ck.cpu().numpy())
    mine, _ = C.kmeans_assign(x[:2000], step.Ck)
    clear = margin > 1e-5
    assert np.array_equal(mine.cpu().numpy()[clear], index[clear])


def test_cpu_tensors_are_refused_on_the_gpu_build():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        C.kmeans_assign(torch.randn(3, 4), torch.randn(2, 4).to(DEV))


# --------------------------------------------------------------------------- against the reference's goldens (g20)
@pytest.fixture(scope="module")
def g20():
    g = np.load(os.path.join(GOLDEN, "g20_kmeans.npz"), allow_pickle=False)
    return g, json.loads(str(g["meta"]))


class _Loader:
    def __init__(self, feats, W=10240):
        self.items = [(torch.zeros(f.shape[0], 1, W), None, torch.from_numpy(f).to(DEV)) for f in feats]

    def __len__(self):
        return len(self.items)

    def __iter__(self):
        return iter(self.items)


def _fm(data):
    return data[2].clone()


def _drop_handlers(name):
    for h in list(C.logging.getLogger(name).handlers):
        C.logging.getLogger(name).removeHandler(h)
        h.close()


def _norm(lines):
    import re
    out = []
    for ln in lines:
        ln = re.sub(r"done in [0-9.]+ seconds", "done in T seconds", ln)
        ln = re.sub(r"Saving last checkpoint to .*/(checkpoint_\d+\.pt)", r"Saving last checkpoint to \1", ln)
        ln = re.sub(r"(checkpoint: |Last diff )\S+", r"\1X", ln)
        out.append(ln)
    return out


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() <= 1e-5 * max(1.0, np.abs(b).max())


def _compare_dir(tmp, g, m, tag):
    assert sorted(os.listdir(tmp)) == m["files"]
    for key, rec in m["checkpoints"].items():
        st = torch.load(os.path.join(tmp, key + ".pt"), map_location="cpu")
        assert sorted(st["state_dict"]) == rec["state_dict_keys"]
        for f in ("n_clusters", "dim", "iteration", "mode"):
            assert st[f] == rec[f], (key, f)
        assert _close(st["last_diff"], rec["last_diff"])
        assert _close(st["state_dict"]["Ck"].cpu().numpy(), g[f"{tag}_{key}_Ck"])


@pytest.mark.parametrize("tag", ["km_init", "km_pis_lo", "km_pis_hi", "km_group2", "km_start_empty", "km_converge"])
def test_kmeangpu_against_reference(g20, tag, tmp_path):
    g, meta = g20
    m = meta[tag]
    start = torch.from_numpy(g[f"{tag}_start"]).to(DEV) if m["start"] else None
    torch.manual_seed(m["seed"])
    try:
        ret = C.kMeanGPU(_Loader(g[f"{tag}_feats"]), _fm, m["k"], n_group=m["n_group"], MAX_ITER=m["MAX_ITER"],
                         EPSILON=m["EPSILON"], perIterSize=m["perIterSize"], start_clusters=start, save_dir=tmp_path,
                         save_last=m["save_last"])
    finally:
        _drop_handlers("Kmean")
    _compare_dir(tmp_path, g, m, tag)
    assert _close(ret.cpu().numpy(), g[f"{tag}_return"])
    logs = open(tmp_path / "training_logs.txt").read().splitlines()
    assert _norm(logs) == _norm(m["file_logs"])                       # same iterations, nItems, files, quirks
    for mine, ref in zip(logs, m["file_logs"]):
        if "checkpoint: " in ref:
            assert _close(float(mine.rsplit(" ", 1)[1]), float(ref.rsplit(" ", 1)[1]))


def test_fastdpmean_against_reference(g20, tmp_path):
    g, meta = g20
    m = meta["dp"]
    try:
        ret = C.fastDPMean(_Loader(g["dp_feats"]), _fm, m["l"], MAX_ITER=m["MAX_ITER"], EPSILON=m["EPSILON"],
                           save_dir=tmp_path, save_last=m["save_last"])
    finally:
        _drop_handlers("DPMean")
    _compare_dir(tmp_path, g, m, "dp")
    assert _close(ret.cpu().numpy(), g["dp_return"])
    logs = open(tmp_path / "training_logs.txt").read().splitlines()
    assert _norm(logs) == _norm(m["logs"])


def test_kmean_against_reference(g20):
    g, meta = g20
    m = meta["kmean"]
    torch.manual_seed(m["seed"])
    ret = C.KMean(torch.from_numpy(g["kmean_C"]).to(DEV), m["k"], MAX_ITER=m["MAX_ITER"])
    assert _close(ret.cpu().numpy(), g["kmean_return"])
    # an empty cluster's mean is NaN, as the reference's: 3 initial rows out of 2 distinct values, so two centroids are
    # equal and the higher index of the pair gets no row
    X = torch.cat([torch.zeros(10, 3), torch.ones(10, 3)]).to(DEV)
    torch.manual_seed(0)
    out = C.KMean(X, 3, MAX_ITER=1)
    assert out.shape == (1, 3, 3) and int(out.isnan().any(dim=2).sum()) == 1


# --------------------------------------------------------------------------- end to end on the committed audio
CKPT = os.path.join(GOLDEN, "ref_checkpoint", "checkpoint_7.pt")
DB = os.path.join(GOLDEN, "test_db")


def _run_script(argv):
    from cpc2_amd.clustering import clustering_script as S
    random.seed(7)
    torch.manual_seed(7)
    try:
        S.main(argv)
    finally:
        _drop_handlers("Kmean")
        _drop_handlers("DPMean")


def test_clustering_script_and_quantization_end_to_end(tmp_path):
    from cpc2_amd.clustering import clustering_quantization as Q
    from cpc2_amd.feature_loader import FeatureModule, buildFeature, loadModel
    out = tmp_path / "clust"
    _run_script([CKPT, str(out), DB, "-k", "4", "-n", "2", "--save"])
    files = sorted(os.listdir(out))
    assert {"args.json", "training_logs.txt", "checkpoint_last.pt", "checkpoint_1.pt"} <= set(files), files
    last = torch.load(out / "checkpoint_last.pt", map_location="cpu")
    assert last["state_dict"]["Ck"].shape == (1, 4, 32) and last["mode"] is None
    args = json.load(open(out / "args.json"))
    assert args["nClusters"] == 4 and args["pathCheckpoint"] == str(os.path.realpath(CKPT))
    logs = open(out / "training_logs.txt").read()
    n_items = [int(v) for v in __import__("re").findall(r"nItems: (\d+)", logs)]
    assert n_items and all(v > 0 and v % 64 == 0 for v in n_items)        # whole windows of 64 frames
    # a second run is bitwise identical
    out2 = tmp_path / "clust2"
    _run_script([CKPT, str(out2), DB, "-k", "4", "-n", "2", "--save"])
    for name in files:
        if name.endswith(".pt"):
            a = torch.load(out / name, map_location="cpu")["state_dict"]["Ck"]
            b = torch.load(out2 / name, map_location="cpu")["state_dict"]["Ck"]
            assert torch.equal(a, b), name
    # an existing directory without --load is refused (nothing written); --load resumes
    before = sorted(os.listdir(out2))
    _run_script([CKPT, str(out2), DB, "-k", "4", "-n", "1"])
    assert sorted(os.listdir(out2)) == before
    _run_script([CKPT, str(out2), DB, "-k", "4", "-n", "1", "--load", str(out / "checkpoint_last.pt")])
    assert "empty clusters out of 4" in open(out2 / "training_logs.txt").read()

    # quantization of every file, against the fp64 oracle on the package's own features
    qdir = tmp_path / "quant"
    Q.main([str(out / "checkpoint_last.pt"), DB, str(qdir)])
    text = open(qdir / "quantized_outputs.txt").read()
    assert not text.endswith("\n")
    lines = dict(ln.split("\t") for ln in text.split("\n"))
    assert len(lines) == 9
    model = loadModel([CKPT])[0]
    fm = FeatureModule(model, False).cuda().eval()
    module = C.loadClusterModule(str(out / "checkpoint_last.pt"))
    ck = module.Ck.cpu().numpy()
    from cpc2_amd.dataset import findAllSeqs
    for _, rel in findAllSeqs(DB, extension=".flac", speaker_level=1)[0]:
        feats = buildFeature(fm, os.path.join(DB, rel), seqNorm=False, strict=True).cuda()
        index, _, margin = KO.assign(feats[0].cpu().numpy(), ck)
        units = np.array([int(u) for u in lines[os.path.splitext(os.path.basename(rel))[0]].split(",")])
        assert len(units) == feats.size(1)
        clear = margin > 1e-5
        assert np.array_equal(units[clear], index[clear])
        assert torch.equal(module.assign(feats), module(feats).argmin(dim=-1))
    with pytest.raises(AssertionError, match="already exists"):
        Q.main([str(out / "checkpoint_last.pt"), DB, str(qdir)])


def test_level_gru_on_a_two_layer_run(tmp_path):
    from cpc2_amd.feature_loader import FeatureModule, loadModel
    from cpc2_amd.model import CPCModel
    from cpc2_amd.train import getAR, getEncoder
    run = tmp_path / "run2"
    run.mkdir()
    args = json.load(open(os.path.join(GOLDEN, "ref_checkpoint", "checkpoint_args.json")))
    args["nLevelsGRU"] = 2
    json.dump(args, open(run / "checkpoint_args.json", "w"))
    shutil.copy(os.path.join(GOLDEN, "ref_checkpoint", "checkpoint_logs.json"), run / "checkpoint_logs.json")
    torch.manual_seed(3)
    two = CPCModel(getEncoder(argparse.Namespace(**args)), getAR(argparse.Namespace(**args)))
    ref_sd = torch.load(CKPT, map_location="cpu")["gEncoder"]
    two.load_state_dict(ref_sd, strict=False)                          # layer 0 from the checkpoint, layer 1 random
    torch.save({"gEncoder": two.state_dict()}, run / "checkpoint_0.pt")
    one = loadModel([str(run / "checkpoint_0.pt")], updateConfig=argparse.Namespace(nLevelsGRU=1))[0]
    full = loadModel([str(run / "checkpoint_0.pt")])[0]
    ref = loadModel([CKPT])[0]
    wave = torch.randn(2, 1, 10240, generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        f1 = FeatureModule(one, False).cuda().eval()((wave, None))
        f0 = FeatureModule(ref, False).cuda().eval()((wave, None))
        f2 = FeatureModule(full, False).cuda().eval()((wave, None))
    assert torch.equal(f1, f0) and not torch.equal(f1, f2)
    out = tmp_path / "clust"
    _run_script([str(run / "checkpoint_0.pt"), str(out), DB, "-k", "2", "-n", "1", "--level_gru", "1"])
    assert json.load(open(out / "args.json"))["level_gru"] == 1
    assert torch.load(out / "checkpoint_last.pt", map_location="cpu")["state_dict"]["Ck"].shape == (1, 2, 32)


def test_model_cluster_combined_formats():
    from cpc2_amd.feature_loader import FeatureModule, ModelClusterCombined, loadModel
    fm = FeatureModule(loadModel([CKPT])[0], False).cuda().eval()
    ck = torch.randn(1, 6, 32, generator=torch.Generator().manual_seed(2)).to(DEV)
    cluster = C.kMeanCluster(ck)
    wave = torch.randn(2, 1, 10240, generator=torch.Generator().manual_seed(4)).to(DEV)
    with torch.no_grad():
        feats = fm((wave, None))
        dist = cluster(feats)
        ids = ModelClusterCombined(fm, cluster, 6, "int")((wave, None))
        one_hot = ModelClusterCombined(fm, cluster, 6, "oneHot")((wave, None))
        soft = ModelClusterCombined(fm, cluster, 6, "softmax")((wave, None))
    assert torch.equal(ids, dist.min(dim=2)[1]) and ids.dtype == torch.long
    assert one_hot.shape == (2, 64, 6) and torch.equal(one_hot.argmax(dim=2), ids) and int(one_hot.sum()) == 128
    assert torch.allclose(soft, torch.softmax(-dist, dim=2))
    with pytest.raises(ValueError, match="Invalid output format"):
        ModelClusterCombined(fm, cluster, 6, "bad")
