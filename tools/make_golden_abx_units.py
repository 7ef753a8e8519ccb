#!/usr/bin/env python3
"""Generate the g22 goldens of the ABX evaluation on quantized units by running the REFERENCE's
cpc/eval/eval_ABX_clustering.py (QuantizedClustering, ClusteringFeatures), its ABX loader / iterators and its Cython DTW on
the CPU:

    tests/golden/g22_quantized_units.txt         six files f0..f5 of 400 units each, 8 units, runs of 1-5 frames
    tests/golden/g22_quantized_units_50.txt      the same with 50 units
    tests/golden/g22_quantized_units_groups.txt  two groups per frame (tokens `a-b`), with g22_onehot_dict.txt
    tests/golden/g22_abx_units.npz               what the reference computes from them (see the keys below)

The item file is the committed g19_abx_synth.item, read only.

    CPC_REFERENCE=<checkout of the reference> PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_abx_units.py

The reference is imported unmodified.  progressbar (a no-op ProgressBar) and torchaudio are stubbed, Tensor.cuda /
Module.cuda are no-ops (the reference's classes call .cuda() unconditionally), and the Cython DTW (dtw.pyx) is compiled by
pyximport into a temporary directory outside the repository.  random.sample is wrapped (by this script) to record every
draw.  For ClusteringFeatures the reference's buildFeature is replaced, inside this tool, by a lookup of a recorded feature
tensor, and its object is assembled without __init__ (which loads a CPC checkpoint); the `onehot` group mode, whose
feature_function reads a global `pair2idx` the reference never defines, gets that name set on the reference's module.  Only
inputs and outputs are written.
"""
import json
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("CPC_REFERENCE")
OUT = os.path.join(ROOT, "tests", "golden")
ITEM = os.path.join(OUT, "g19_abx_synth.item")
if not REF or not os.path.isdir(os.path.join(REF, "cpc")):
    raise SystemExit("set CPC_REFERENCE to a checkout of the reference (the directory that holds cpc/)")


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
for _name in ("tqdm", "psutil"):
    try:
        __import__(_name)
    except ImportError:
        sys.modules[_name] = types.ModuleType(_name)
torch.Tensor.cuda = lambda self, *a, **k: self
torch.nn.Module.cuda = lambda self, *a, **k: self
import pyximport  # noqa: E402

_BUILD = tempfile.mkdtemp(prefix="abx_dtw_build_")
pyximport.install(build_dir=_BUILD, setup_args={"include_dirs": np.get_include()}, language_level=3)
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REF, "cpc", "eval"))
import ABX.abx_group_computation as ref_g  # noqa: E402
import ABX.abx_iterators as ref_it  # noqa: E402
import eval_ABX as ref_eval  # noqa: E402
import cpc.eval.eval_ABX_clustering as ref_c  # noqa: E402
from cpc.clustering.clustering import kMeanCluster as RefCluster  # noqa: E402

torch.set_num_threads(8)
ARR = {}
DRAWS = []
_sample = random.sample


def _recording_sample(population, k):
    out = _sample(population, k=k)
    DRAWS.append(json.dumps([list(v) if isinstance(v, tuple) else v for v in out]))
    return out


random.sample = _recording_sample
SEED, STEP, MAX_SIZE_GROUP, MAX_X_ACROSS = 2201, 100.0, 10, 5      # the last two: eval_ABX_Librispeech's settings
N_GROUP_IDS = 6                                                   # ids per group of the two-group variant


# --------------------------------------------------------------------------- unit files
def runs(rng, n_frames, n_units):
    out = []
    while len(out) < n_frames:
        out += [int(rng.integers(0, n_units))] * int(rng.integers(1, 6))
    return out[:n_frames]


def write_units(name, rng, n_units, groups=False):
    lines = []
    for f in range(6):
        if groups:
            a, b = runs(rng, 400, N_GROUP_IDS), runs(rng, 400, N_GROUP_IDS)
            lines.append(f"f{f}\t" + ",".join(f"{i}-{j}" for i, j in zip(a, b)))
        else:
            lines.append(f"f{f}\t" + ",".join(str(u) for u in runs(rng, 400, n_units)))
    path = os.path.join(OUT, name)
    with open(path, "w") as fh:
        fh.write("\n".join(lines))                     # no trailing newline, as clustering_quantization writes it
    return path


def write_dict(name):
    path = os.path.join(OUT, name)
    tokens = [f"{i}-{j}" for i in range(N_GROUP_IDS) for j in range(N_GROUP_IDS)]
    with open(path, "w") as fh:
        fh.write("\n".join(f"{t} {100 - k}" for k, t in enumerate(tokens)) + "\n")
    return path


# --------------------------------------------------------------------------- whole evaluation
def abx_case(tag, quantized, onehot_dict):
    qc = ref_c.QuantizedClustering(quantized, onehot_dict=onehot_dict)
    seq_list = [(f"f{f}", f"f{f}.flac") for f in range(6)]
    ARR[f"{tag}_cfg"] = np.array([SEED, STEP, MAX_SIZE_GROUP, MAX_X_ACROSS, qc.n_units])
    DRAWS.clear()
    random.seed(SEED)
    ds = ref_it.ABXFeatureLoader(ITEM, seq_list, qc.feature_function, STEP, True)
    ARR[f"{tag}_features"] = np.array(ds.features, dtype=np.float64)
    data = ds.data.numpy()
    assert data.shape[1] == qc.n_units + 1
    ARR[f"{tag}_data_units"] = data[:, :qc.n_units].argmax(1).astype(np.int16)
    ARR[f"{tag}_data_values"] = np.unique(data)                  # 0, 1e-12 and 1: nothing else
    for mode in ("within", "across"):
        it = ds.get_iterator(mode, MAX_SIZE_GROUP, MAX_X_ACROSS)
        sp = ref_g.get_abx_scores_dtw_on_group(it, ref_g.get_cosine_distance_batch, it.symmetric)
        ARR[f"{tag}_{mode}_coords"] = sp._indices().numpy().T.astype(np.int16)
        ARR[f"{tag}_{mode}_values"] = sp._values().numpy()
        ARR[f"{tag}_{mode}_board"] = np.array(sp.size())
    ARR[f"{tag}_draws"] = np.array(list(DRAWS))
    random.seed(SEED)
    scores = ref_eval.ABX(qc.feature_function, ITEM, seq_list, "cosine", STEP, ["within", "across"], cuda=False,
                          max_x_across=MAX_X_ACROSS, max_size_group=MAX_SIZE_GROUP, normalize=True)
    ARR[f"{tag}_scores"] = np.array([scores["within"], scores["across"]])
    print(tag, scores, len(DRAWS), "draws", flush=True)


# --------------------------------------------------------------------------- DTW cases on unit sequences
def expand(units, n_units):
    """The loader's rows of one item: one-hot [1, L, n_units] through the reference's normalisation."""
    rows = torch.zeros(1, len(units), n_units)
    rows.scatter_(-1, torch.tensor(units).view(1, -1, 1), 1)
    return ref_it.normalize_with_singularity(rows)[0]


def padded(items, n_units):
    S = max(len(u) for u in items)
    x = torch.zeros(len(items), S, n_units + 1)
    pad = np.full((len(items), S), -1, dtype=np.int16)
    for i, u in enumerate(items):
        x[i, :len(u)] = expand(u, n_units)
        pad[i, :len(u)] = u
    return x, torch.tensor([len(u) for u in items]), pad


def dtw_cases():
    rng = np.random.default_rng(2202)
    cases = [([1, 2, 63], [1, 64, 65, 200], 8, 0, False),
             ([65, 64, 200, 5], None, 2, 0, True),
             ([2, 64, 200], [1, 63, 65], 50, 1, False),
             ([63, 65, 7, 1], None, 8, 1, True)]
    for k, (l1, l2, n_units, code, sym) in enumerate(cases):
        xs = [runs(rng, n, n_units) for n in l1]
        ys = xs if sym else [runs(rng, n, n_units) for n in l2]
        a, sa, pa = padded(xs, n_units)
        b, sb, pb = padded(ys, n_units)
        fn = ref_g.get_cosine_distance_batch if code == 0 else ref_g.get_euclidian_distance_batch
        out = ref_g.get_distance_group_dtw(a, b, sa, sb, ignore_diag=sym, symmetric=sym, distance_function=fn)
        ARR[f"dtw{k}_x"], ARR[f"dtw{k}_y"] = pa, pb
        ARR[f"dtw{k}_cfg"] = np.array([code, int(sym), n_units])
        ARR[f"dtw{k}_out"] = out.numpy()
    ARR["dtw_n"] = np.array(len(cases))


# --------------------------------------------------------------------------- ClusteringFeatures
def clustering_cases(onehot_dict):
    rng = np.random.default_rng(2203)
    k, d, S = N_GROUP_IDS, 4, 40
    ck = torch.from_numpy(rng.standard_normal((1, k, d)).astype(np.float32))
    ARR["cf_Ck"] = ck.numpy()
    recorded = {}
    ref_c.buildFeature = lambda feature_maker, x, **kw: recorded[x].clone()
    with open(onehot_dict, "r") as f:
        ref_c.pair2idx = {word.split()[0]: i for i, word in enumerate(f.read().split("\n")) if word}
    for n_groups in (1, 2):
        pick = rng.integers(0, k, size=S * n_groups)
        feat = ck[0, pick] + torch.from_numpy((0.02 * rng.standard_normal((S * n_groups, d))).astype(np.float32))
        sq = ((feat.double().view(-1, 1, d) - ck.double()) ** 2).sum(2).sort(dim=1).values
        margin = float(((sq[:, 1] - sq[:, 0]) / sq[:, 1]).min())
        assert margin >= 1e-3, margin                    # the assignment cannot hang on summation order
        recorded["x"] = feat.view(1, S, d * n_groups)
        ARR[f"cf_g{n_groups}_feat"] = recorded["x"].numpy()
        ARR[f"cf_g{n_groups}_margin"] = np.array(margin)
        for soft, mode in [(True, "concat")] + [(False, m) for m in ("seq", "onehot", "concat", "combine")]:
            cf = object.__new__(ref_c.ClusteringFeatures)
            cf.group_modes, cf.soft_clustering, cf.featureMaker = mode, soft, None
            cf.clusterModule = RefCluster(ck.clone())
            cf.dim_clusters, cf.n_groups = d, n_groups
            out = cf.feature_function("x")
            ARR[f"cf_g{n_groups}_{'soft' if soft else mode}"] = out.numpy() if soft else out.numpy().astype(np.uint8)
            ARR[f"cf_g{n_groups}_{'soft' if soft else mode}_step"] = np.array(cf.step_feature_multiplication)


def main():
    rng = np.random.default_rng(2204)
    u8 = write_units("g22_quantized_units.txt", rng, 8)
    u50 = write_units("g22_quantized_units_50.txt", rng, 50)
    ug = write_units("g22_quantized_units_groups.txt", rng, 0, groups=True)
    dic = write_dict("g22_onehot_dict.txt")
    abx_case("u8", u8, None)
    abx_case("u50", u50, None)
    abx_case("ug", ug, dic)
    dtw_cases()
    clustering_cases(dic)
    ARR["torch_version"] = np.array(torch.__version__)
    np.savez_compressed(os.path.join(OUT, "g22_abx_units.npz"), **ARR)
    print("wrote g22_abx_units.npz", os.path.getsize(os.path.join(OUT, "g22_abx_units.npz")), "bytes")


if __name__ == "__main__":
    main()
