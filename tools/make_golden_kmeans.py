#!/usr/bin/env python3
"""Generate tests/golden/g20_kmeans.npz and g20_quantized_outputs.txt by running the REFERENCE's clustering
(cpc/clustering/clustering.py, clustering_quantization.py) on the CPU.

Runs only in the build container where /root/reference exists:
    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_kmeans.py

The reference is imported unmodified.  progressbar (a no-op ProgressBar) and torchaudio are stubbed, Tensor.cuda and
Module.cuda are the identity, and nn.DataParallel without a device calls its module directly.  The feature maker and the
data loader serve fixed synthetic feature batches: Gaussian blobs far apart.  Every assignment of every iteration is
checked against the fp64 oracle (tests/kmeans_oracle.py): its relative best-versus-second gap must be at least 1e-3, so
f32 summation order cannot flip it; every last_diff must be far (x10) from EPSILON, and every DP-means max distance far
from lambda.  Only inputs and outputs are written.
"""
import contextlib
import io
import json
import logging
import os
import shutil
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kmeans_oracle as KO  # noqa: E402


class _ProgressBar:
    def __init__(self, *a, **k):
        pass

    def start(self):
        pass

    def update(self, *a):
        pass

    def finish(self):
        pass


sys.modules["progressbar"] = types.SimpleNamespace(ProgressBar=_ProgressBar)
sys.modules.setdefault("torchaudio", types.ModuleType("torchaudio"))
torch.Tensor.cuda = lambda self, *a, **k: self
torch.nn.Module.cuda = lambda self, *a, **k: self
sys.path.insert(0, REF)
import cpc.clustering.clustering as ref_cl  # noqa: E402
import cpc.clustering.clustering_quantization as ref_q  # noqa: E402

ARR = {}
META = {}
MARGIN = 1e-3


def blobs(rng, n_batches, B, S, D, centers, spread):
    """n_batches feature batches [B, S, D]: every frame a center plus Gaussian noise."""
    out = []
    for _ in range(n_batches):
        pick = rng.integers(0, len(centers), size=(B, S))
        out.append((centers[pick] + spread * rng.standard_normal((B, S, D))).astype(np.float32))
    return out


class Loader:
    """What kMeanGPU reads of a batch: data[0] ([B, 1, W] samples, for sum_seen) and the features in data[2]."""

    def __init__(self, feats, W=10240):
        self.items = [(torch.zeros(f.shape[0], 1, W), torch.zeros(f.shape[0], dtype=torch.long), torch.from_numpy(f))
                      for f in feats]

    def __len__(self):
        return len(self.items)

    def __iter__(self):
        return iter(self.items)


def feature_maker(data):
    return data[2].clone()


@contextlib.contextmanager
def recording_step():
    """Check the margin of every kMeanClusterStep assignment (the reference's own forward runs unchanged)."""
    orig = ref_cl.kMeanClusterStep.forward

    def forward(self, locF):
        _, _, margin = KO.assign(locF.view(locF.size(0), -1).numpy(), self.Ck.numpy())
        assert margin.min() >= MARGIN, f"assignment margin {margin.min():.2e} below {MARGIN}"
        return orig(self, locF)

    ref_cl.kMeanClusterStep.forward = forward
    try:
        yield
    finally:
        ref_cl.kMeanClusterStep.forward = orig


def capture_logs(name):
    buf = io.StringIO()
    h = logging.StreamHandler(buf)
    h.setFormatter(logging.Formatter("%(message)s"))
    logging.getLogger(name).addHandler(h)
    return buf, h


def read_dir(d, tag, eps):
    """Every checkpoint left in d: its arrays into ARR, the rest into the returned dict."""
    out = {}
    names = sorted(os.listdir(d))
    for name in names:
        if not name.startswith("checkpoint_"):
            continue
        st = torch.load(os.path.join(d, name), map_location="cpu")
        key = name[:-3]
        ARR[f"{tag}_{key}_Ck"] = st["state_dict"]["Ck"].numpy()
        out[key] = {k: v for k, v in st.items() if k != "state_dict"}
        out[key]["state_dict_keys"] = sorted(st["state_dict"])
        if st["last_diff"] is not None:
            ld = st["last_diff"]
            assert not (eps / 10 <= ld <= eps * 10), f"{tag}: last_diff {ld} too close to EPSILON {eps}"
    return names, out


def lines(text, save_dir):
    """Log lines with the temporary output directory written as SAVE_DIR."""
    return text.replace(save_dir, "SAVE_DIR").splitlines()


def save_feats(tag, feats):
    ARR[f"{tag}_feats"] = np.stack(feats)


def kmean_case(tag, seed, feats, k, n_group=1, MAX_ITER=6, EPSILON=1e-4, perIterSize=-1, start=None, save_last=3):
    save_feats(tag, feats)
    if start is not None:
        ARR[f"{tag}_start"] = start
    d = tempfile.mkdtemp(prefix="g20_")
    torch.manual_seed(seed)
    buf, h = capture_logs("Kmean")
    with recording_step(), contextlib.redirect_stdout(io.StringIO()) as out:
        ret = ref_cl.kMeanGPU(Loader(feats), feature_maker, k, n_group=n_group, MAX_ITER=MAX_ITER, EPSILON=EPSILON,
                              perIterSize=perIterSize, start_clusters=None if start is None else torch.from_numpy(start),
                              save_dir=d, save_last=save_last)
    logging.getLogger("Kmean").removeHandler(h)
    for hh in list(logging.getLogger("Kmean").handlers):
        logging.getLogger("Kmean").removeHandler(hh)
    names, ckpts = read_dir(d, tag, EPSILON)
    with open(os.path.join(d, "training_logs.txt")) as f:
        file_logs = f.read()
    ARR[f"{tag}_return"] = ret.numpy()
    META[tag] = dict(kind="kMeanGPU", seed=seed, k=k, n_group=n_group, MAX_ITER=MAX_ITER, EPSILON=EPSILON,
                     perIterSize=perIterSize, save_last=save_last, start=start is not None, files=names,
                     checkpoints=ckpts, logs=lines(buf.getvalue(), d), file_logs=lines(file_logs, d),
                     stdout=lines(out.getvalue(), d))
    shutil.rmtree(d)


def dpmean_case(tag, feats, l, MAX_ITER=5, EPSILON=1e-4, save_last=3):
    save_feats(tag, feats)
    # the oracle's own replay: margins of every assignment, distance to lambda of every max
    init = sum(f.astype(np.float64) for f in feats[:102]) if len(feats) <= 102 else None
    mu = init.reshape(-1, init.shape[-1]).mean(axis=0, keepdims=True) / 100
    for _ in range(MAX_ITER):
        sums, counts = np.zeros_like(mu), np.zeros(mu.shape[0], np.int64)
        for f in feats:
            x = f.reshape(-1, f.shape[-1])
            _, best, margin = KO.assign(x, mu)
            assert margin.min() >= MARGIN or mu.shape[0] == 1
            dmax = np.sqrt(best).max()
            assert abs(dmax - l) / l > MARGIN, (dmax, l)
            index, mu, added = KO.dpmeans_batch(x, mu, l)
            if added:
                sums = np.concatenate([sums, np.zeros((1, mu.shape[1]))])
                counts = np.concatenate([counts, [0]])
            s, c = KO.sums_counts(x, index, mu.shape[0])
            sums, counts = sums + s, counts + c
        new = sums / (counts[:, None] + 1e-4)
        ld = np.sqrt(((mu - new) ** 2).sum(1)).max()
        mu = new
        if ld < EPSILON:
            break
    d = tempfile.mkdtemp(prefix="g20_")
    buf, h = capture_logs("DPMean")
    with contextlib.redirect_stdout(io.StringIO()):
        ret = ref_cl.fastDPMean(Loader(feats), feature_maker, l, MAX_ITER=MAX_ITER, EPSILON=EPSILON, save_dir=d,
                                save_last=save_last)
    for hh in list(logging.getLogger("DPMean").handlers):
        logging.getLogger("DPMean").removeHandler(hh)
    names, ckpts = read_dir(d, tag, EPSILON)
    ARR[f"{tag}_return"] = ret.numpy()
    META[tag] = dict(kind="fastDPMean", l=l, MAX_ITER=MAX_ITER, EPSILON=EPSILON, save_last=save_last, files=names,
                     checkpoints=ckpts, logs=lines(buf.getvalue(), d))
    shutil.rmtree(d)


def kmean_plain_case(tag, seed, C, k, MAX_ITER=20):
    ARR[f"{tag}_C"] = C
    torch.manual_seed(seed)
    perm = torch.randperm(C.shape[0])[:k].numpy()
    ck = C[perm].astype(np.float64)
    for _ in range(MAX_ITER):                        # margins along the oracle's trajectory
        idx, _, margin = KO.assign(C, ck)
        assert margin.min() >= MARGIN
        s, c = KO.sums_counts(C, idx, k)
        new = s / c[:, None]
        if np.sqrt(((ck - new) ** 2).sum(1)).max() < 1e-4:
            break
        ck = new
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()) as out:
        ret = ref_cl.KMean(torch.from_numpy(C), k, MAX_ITER=MAX_ITER)
    ARR[f"{tag}_return"] = ret.numpy()
    META[tag] = dict(kind="KMean", seed=seed, k=k, MAX_ITER=MAX_ITER, stdout=out.getvalue().splitlines())


def first_passing(make, seeds):
    for s in seeds:
        try:
            return make(s)
        except AssertionError as e:
            print(f"  seed {s} rejected: {e}")
    raise RuntimeError("no seed passed the margin checks")


def quantization_case():
    """clustering_quantization.main with the model replaced by recorded features: the output file, byte for byte."""
    rng = np.random.default_rng(2020)
    d, nGroups, k = 6, 2, 5
    centers = rng.uniform(-8, 8, size=(k, d))
    ck = (centers + 0.05 * rng.standard_normal((k, d))).astype(np.float32)
    tmp = tempfile.mkdtemp(prefix="g20q_")
    db = os.path.join(tmp, "db")
    for spk, names in (("s1", ["a_1", "a_2", "a_3"]), ("s2", ["b_1", "b_2"]), ("s3", ["c_1", "c_2"])):
        os.makedirs(os.path.join(db, spk))
        for n in names:
            open(os.path.join(db, spk, n + ".flac"), "w").close()
    run = os.path.join(tmp, "clust")
    os.makedirs(run)
    with open(os.path.join(run, "args.json"), "w") as f:
        json.dump(dict(pathCheckpoint="unused.pt", encoder_layer=False, level_gru=None, train_mode=False,
                       dimReduction=None, centroidLimits=None), f)
    feats = {}
    for root, _, files in os.walk(db):
        for fn in files:
            if fn.endswith(".flac"):
                S = int(rng.integers(3, 9))
                pick = rng.integers(0, k, size=S * nGroups)
                feats[fn[:-5]] = (centers[pick] + 0.3 * rng.standard_normal((S * nGroups, d))).astype(np.float32) \
                    .reshape(1, S, nGroups * d)
    for name, f in feats.items():
        _, _, margin = KO.assign(f.reshape(-1, d), ck)
        assert margin.min() >= MARGIN
        ARR[f"q_feat_{name}"] = f
    ARR["q_Ck"] = ck.reshape(1, k, d)

    class FakeModel:
        gAR = types.SimpleNamespace(keepHidden=False)

    class FakeFeature:
        def eval(self):
            return self

        def cuda(self):
            return self

    seqs = {}
    orig_find = ref_q.findAllSeqs

    def find(*a, **kw):
        out = orig_find(*a, **kw)
        seqs["list"] = [list(v) for v in out[0]]
        return out

    ref_q.findAllSeqs = find
    ref_q.loadModel = lambda paths, updateConfig=None: (FakeModel(), 0, 0)
    ref_q.FeatureModule = lambda model, enc: FakeFeature()
    ref_q.buildFeature = lambda fm, path, seqNorm=False, strict=False: torch.from_numpy(
        feats[os.path.splitext(os.path.basename(path))[0]])
    ref_q.loadClusterModule = lambda path: ref_cl.kMeanCluster(torch.from_numpy(ck.reshape(1, k, d)))
    outs = {}
    for split in (None, "2-3", "3-3"):
        o = os.path.join(tmp, f"out_{split}")
        argv = [os.path.join(run, "checkpoint_last.pt"), db, o] + ([] if split is None else ["--split", split])
        with contextlib.redirect_stdout(io.StringIO()):
            ref_q.main(argv)
        name = "quantized_outputs.txt" if split is None else f"quantized_outputs_split_{split}.txt"
        with open(os.path.join(o, name), "rb") as f:
            outs[split or "all"] = f.read().decode()
    META["quantization"] = dict(seqNames=seqs["list"], nGroups=nGroups, splits=outs)
    with open(os.path.join(OUT, "g20_quantized_outputs.txt"), "wb") as f:
        f.write(outs["all"].encode())
    shutil.rmtree(tmp)


def parse_defaults():
    sys.modules.setdefault("cpc.criterion.research", types.ModuleType("cpc.criterion.research"))
    dr = types.ModuleType("cpc.criterion.research.dim_reduction")
    dr.loadDimReduction = None
    sys.modules.setdefault("cpc.criterion.research.dim_reduction", dr)
    import cpc.clustering.clustering_script as ref_s
    a = vars(ref_s.parseArgs(["ckpt.pt", "out", "db"]))
    b = vars(ref_q.parseArgs(["ckpt.pt", "db", "out"]))
    c = vars(ref_q.parseArgs(["ckpt.pt", "db", "out", "--strict", "False"]))
    META["defaults"] = dict(clustering_script=a, clustering_quantization=b, quantization_strict_false=c)


def main():
    rng = np.random.default_rng(20)
    D = 8
    centers = rng.uniform(-10, 10, size=(4, D))
    # plain k-means from a random init, 1 group; the same with perIterSize below / above the loader length
    first_passing(lambda s: kmean_case("km_init", s, blobs(np.random.default_rng(100 + s), 8, 2, 16, D, centers, 0.5),
                                       4, MAX_ITER=5), range(20))
    first_passing(lambda s: kmean_case("km_pis_lo", s, blobs(np.random.default_rng(200 + s), 8, 2, 16, D, centers, 0.5),
                                       4, MAX_ITER=4, perIterSize=3), range(20))
    first_passing(lambda s: kmean_case("km_pis_hi", s, blobs(np.random.default_rng(300 + s), 5, 2, 16, D, centers, 0.5),
                                       4, MAX_ITER=3, perIterSize=7), range(20))
    # two groups: frames of 2 x D split into rows of D
    first_passing(lambda s: kmean_case("km_group2", s, blobs(np.random.default_rng(400 + s), 8, 2, 12, 2 * D,
                                                              np.concatenate([centers, centers[::-1]], axis=1), 0.5),
                                       4, n_group=2, MAX_ITER=4), range(20))
    # given start clusters, one far from every blob: it stays empty (zero vector after the update)
    start = np.concatenate([centers[:3] + 0.3, np.full((1, D), 60.0)]).astype(np.float32).reshape(1, 4, D)
    first_passing(lambda s: kmean_case("km_start_empty", s, blobs(np.random.default_rng(500 + s), 6, 2, 16, D,
                                                                   centers[:3], 0.5), 4, MAX_ITER=4, start=start),
                  range(20))
    # converging run: start at the blob centres, stops at iteration 2 and returns the previous centroids
    start2 = (centers + 0.2).astype(np.float32).reshape(1, 4, D)
    first_passing(lambda s: kmean_case("km_converge", s, blobs(np.random.default_rng(600 + s), 6, 2, 16, D, centers, 0.4),
                                       4, MAX_ITER=20, start=start2, save_last=2), range(20))
    # DP-means: lambda between the blob spread and the blob distances
    first_passing(lambda s: dpmean_case("dp", blobs(np.random.default_rng(700 + s), 6, 2, 16, D, centers, 0.3), 6.0),
                  range(20))
    # KMean on rows
    first_passing(lambda s: kmean_plain_case("kmean", s, blobs(np.random.default_rng(800 + s), 1, 1, 300, D, centers,
                                                                0.5)[0].reshape(-1, D), 4), range(20))
    quantization_case()
    parse_defaults()
    ARR["meta"] = np.array(json.dumps(META, default=str))
    np.savez_compressed(os.path.join(OUT, "g20_kmeans.npz"), **ARR)
    print("wrote", os.path.join(OUT, "g20_kmeans.npz"), os.path.getsize(os.path.join(OUT, "g20_kmeans.npz")), "bytes")


if __name__ == "__main__":
    main()
