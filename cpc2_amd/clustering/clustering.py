"""k-means and DP-means on CPC features -- cpc/clustering/clustering.py of the reference, same names, signatures,
checkpoint layout and log lines, computed by the kernels of csrc/kmeans.hip:

  kmeans_assign       fused distance + argmin (never the [n, k] matrix), the lowest index among equal minima
  kmeans_distances    the full [n, k] sums of squares, bit-identical to what assign compares
  kmeans_accumulate   running per-cluster sums and counts, bitwise reproducible (no float atomic)

Every distance is the f32 chain sum_d (x - c)^2 in ascending d.  GPU tensors only: there is no CPU path.  The reference's
quirks are kept on purpose: kMeanGPU returns the PREVIOUS centroids when it converges, always logs
"ended in MAX_ITER", and re-enters its loop (zeroing the running sums) when the loader ends before perIterSize batches;
fastDPMean divides its initial mean by 100 and regularises the counts by 1e-4; KMean leaves an empty cluster at NaN.
"""
import logging
from os import remove
from pathlib import Path
from time import time

import torch
import torch.nn as nn

from .. import _lib


# --------------------------------------------------------------------------- kernels
def _device():
    return torch.device("cuda", torch.cuda.current_device())


def _rows(x, d, what):
    _lib.require_gpu(x)
    x = _lib.f32c(x)
    if x.size(-1) != d:
        raise ValueError(f"{what}: features of width {x.size(-1)} against centroids of width {d}")
    return x.view(-1, d)


def kmeans_assign(x, ck, want_min_sq=True):
    """(index [n] int32, min_sq [n] f32 or None) of the rows x [..., d] against the centroids ck [..., k, d]."""
    _lib.require_gpu(ck)
    ck = _lib.f32c(ck)
    d = ck.size(-1)
    ck = ck.view(-1, d)
    x = _rows(x, d, "kmeans_assign")
    n, k = x.size(0), ck.size(0)
    index = torch.empty(n, dtype=torch.int32, device=x.device)
    min_sq = torch.empty(n, dtype=torch.float32, device=x.device) if want_min_sq else None
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().cpc_kmeans_assign(_lib.ptr(x), n, d, _lib.ptr(ck), k, _lib.ptr(index), _lib.ptr(min_sq),
                                                 _lib.stream_ptr(x.device)), "kmeans_assign")
    return index, min_sq


def kmeans_distances(x, ck):
    """[n, k] sums of squares of the rows x [..., d] against the centroids ck [..., k, d]."""
    _lib.require_gpu(ck)
    ck = _lib.f32c(ck)
    d = ck.size(-1)
    ck = ck.view(-1, d)
    x = _rows(x, d, "kmeans_distances")
    n, k = x.size(0), ck.size(0)
    dist = torch.empty(n, k, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().cpc_kmeans_distances(_lib.ptr(x), n, d, _lib.ptr(ck), k, _lib.ptr(dist),
                                                    _lib.stream_ptr(x.device)), "kmeans_distances")
    return dist


def kmeans_accumulate(x, index, sums, counts):
    """sums [..., k, d] += per-cluster row sums of x [..., d] by index (int32, one per row); counts [k] (int64) += rows.
    A row whose index is outside [0, k) is skipped.  In place, bitwise reproducible."""
    _lib.require_gpu(index, sums, counts)
    d = sums.size(-1)
    if not sums.is_contiguous() or sums.dtype != torch.float32:
        raise TypeError("kmeans_accumulate: sums must be a contiguous fp32 tensor")
    if counts.dtype != torch.int64 or not counts.is_contiguous():
        raise TypeError("kmeans_accumulate: counts must be a contiguous int64 tensor")
    k = counts.numel()
    if sums.numel() != k * d:
        raise ValueError(f"kmeans_accumulate: sums of {sums.numel()} elements for {k} clusters of width {d}")
    x = _rows(x, d, "kmeans_accumulate")
    if index.dtype != torch.int32:
        raise TypeError(f"kmeans_accumulate: index must be int32 (got {index.dtype})")
    index = index.contiguous().view(-1)
    if index.numel() != x.size(0):
        raise ValueError(f"kmeans_accumulate: {index.numel()} indices for {x.size(0)} rows")
    lib = _lib.load()
    n = x.size(0)
    need = lib.cpc_kmeans_scratch_bytes(n, d, k)
    with torch.cuda.device(x.device):
        buf = _lib.scratch(need, x.device)
        _lib.check(lib.cpc_kmeans_accumulate(_lib.ptr(x), n, d, _lib.ptr(index), k, _lib.ptr(sums), _lib.ptr(counts),
                                             _lib.ptr(buf), buf.numel(), _lib.stream_ptr(x.device)), "kmeans_accumulate")
    return sums, counts


# --------------------------------------------------------------------------- modules
def loadClusterModule(pathCheckpoint):
    """clustering.py:16-21; loaded to the host first, so a checkpoint saved with CUDA tensors loads anywhere."""
    print(f"Loading ClusterModule at {pathCheckpoint}")
    state_dict = torch.load(pathCheckpoint, map_location="cpu")
    clusterModule = kMeanCluster(state_dict["state_dict"]["Ck"])
    clusterModule = clusterModule.cuda()
    return clusterModule


class kMeanCluster(nn.Module):
    """clustering.py:24-34: forward(features [B, S, d]) -> [B, S, k] sums of squares (kmeans_distances)."""

    def __init__(self, Ck):
        super(kMeanCluster, self).__init__()
        self.register_buffer("Ck", Ck)
        self.k = Ck.size(1)

    def forward(self, features):
        B, S, D = features.size()
        return kmeans_distances(features.contiguous().view(B * S, -1), self.Ck).view(-1, S, self.k)

    def assign(self, features):
        """[B, S] int64: the argmin of forward(features) over the centroids, from the fused kernel."""
        B, S, D = features.size()
        index, _ = kmeans_assign(features.contiguous().view(B * S, -1), self.Ck, want_min_sq=False)
        return index.view(B, S).long()


class kMeanClusterStep(torch.nn.Module):
    """clustering.py:37-55: forward(locF [n, 1, D]) -> (Ck1 [1, k, D] per-cluster SUMS, nItems [1, k])."""

    def __init__(self, k, D):
        super(kMeanClusterStep, self).__init__()
        self.k = k
        self.register_buffer("Ck", torch.zeros(1, k, D))

    def accumulate(self, locF, Ck1, nItems):
        """Ck1 [1, k, D] += sums, nItems [k] += counts of locF's rows, on the device (no host synchronisation)."""
        index, _ = kmeans_assign(locF, self.Ck, want_min_sq=False)
        kmeans_accumulate(locF, index, Ck1, nItems)

    def forward(self, locF):
        Ck1 = torch.zeros(self.Ck.size(), device=self.Ck.device)
        nItems = torch.zeros(self.k, dtype=torch.long, device=self.Ck.device)
        self.accumulate(locF, Ck1, nItems)
        return Ck1, nItems.view(1, -1)


def save_cluster_step(Ck: torch.tensor, path_out: Path, mode: str = None, iter: int = None, last_diff: float = None):
    out_state_dict = {}
    out_state_dict["state_dict"] = {"Ck": Ck}
    out_state_dict["n_clusters"] = Ck.size(1)
    out_state_dict["dim"] = Ck.size(2)
    out_state_dict["iteration"] = iter
    out_state_dict["last_diff"] = last_diff
    out_state_dict["mode"] = mode
    torch.save(out_state_dict, path_out)


def get_last_checkpoint(path_in: Path):
    checkpoint_list = list(Path(path_in).glob("checkpoint_*.pt"))
    valid_paths = [x for x in checkpoint_list if x.stem.split("_")[-1].isdigit()]
    valid_paths.sort(key=lambda x: int(x.stem.split("_")[-1]))
    if len(valid_paths) == 0:
        raise RuntimeError("No checkpoint found")
    return valid_paths[-1]


def setup_log_file(save_dir: Path):
    path_logs = Path(save_dir) / "training_logs.txt"
    return logging.FileHandler(path_logs)


def _save_step(save_dir, iter, save_last, Ck, last_diff, mode, logger):
    path_save = save_dir / f"checkpoint_{iter}.pt"
    logger.info(f"Saving last checkpoint to {path_save}")
    save_cluster_step(Ck, path_save, iter=iter, last_diff=last_diff, mode=mode)
    if (save_dir / f"checkpoint_{iter-save_last}.pt").is_file():
        remove(save_dir / f"checkpoint_{iter-save_last}.pt")


# --------------------------------------------------------------------------- algorithms
def kMeanGPU(dataLoader, featureMaker, k, n_group=1, MAX_ITER=100, EPSILON=1e-4, perIterSize=-1, start_clusters=None,
             save_dir=None, save_last=5):
    """clustering.py:90-205 on one GPU: per batch featureMaker, assign and accumulate into running sums and counts on the
    device; one host synchronisation per iteration."""
    logging.basicConfig(level=logging.INFO)
    logger = logging.getLogger("Kmean")
    logger.setLevel(logging.INFO)          # (basicConfig does nothing when the root logger already has a handler)
    save = save_dir is not None
    if save:
        save_dir = Path(save_dir)
        logger.addHandler(setup_log_file(save_dir))

    logger.info(f"Start Kmean clustering with {k} clusters and {n_group} groups...")
    device = _device()

    if start_clusters is None:
        Ck = []
        with torch.no_grad():
            for index, data in enumerate(dataLoader):
                cFeature = featureMaker(data)
                cFeature = cFeature.contiguous().view(-1, cFeature.size(2) // n_group)
                Ck.append(cFeature)
                if index > k:
                    break
        Ck = torch.cat(Ck, dim=0)
        N, D = Ck.size()
        indexes = torch.randperm(N)[:k]
        Ck = Ck[indexes.to(Ck.device)].view(1, k, D)
    else:
        Ck = start_clusters
        D = Ck.size(2)

    if perIterSize < 0:
        perIterSize = len(dataLoader)

    clusterStep = kMeanClusterStep(k, D).to(device)
    clusterStep.Ck.copy_(Ck)

    iter, stored = 0, 0
    sum_seen = 0
    print("perIterSize = %.f" % perIterSize)
    with torch.no_grad():
        while iter < MAX_ITER:
            start_time = time()
            Ck1 = torch.zeros(Ck.size(), device=device)
            nItemsClusters = torch.zeros(Ck.size(1), dtype=torch.long, device=device)
            for index, data in enumerate(dataLoader):
                cFeature = featureMaker(data).contiguous().view(-1, 1, D)
                clusterStep.accumulate(cFeature, Ck1, nItemsClusters)
                stored += 1
                sum_seen += data[0].shape[0] * data[0].shape[-1] / 16000
                if stored >= perIterSize:
                    break

            if stored < perIterSize:
                # the loader ended first: the loop starts over, running sums zeroed, `stored` kept (as the reference)
                continue

            stored = 0
            iter += 1
            print("I've seen %.2f hours in %d epochs :) More data more data more data!" % (sum_seen / 3600, iter))

            nItemsClusters = nItemsClusters.float().view(1, -1, 1) + 1e-8
            Ck1 /= nItemsClusters
            last_diff, nItems = torch.stack([(clusterStep.Ck - Ck1).norm(dim=2).max(), nItemsClusters.sum()]).tolist()
            nItems = int(nItems)
            logger.info(
                f"ITER {iter} done in {time()-start_time:.2f} seconds. nItems: {nItems}. Difference with last checkpoint: {last_diff}"
            )

            if save:
                _save_step(save_dir, iter, save_last, Ck1, last_diff, "kMean", logger)
            if last_diff < EPSILON:
                logger.info(f"Clustering ended in {iter} iterations out of {MAX_ITER}")
                break
            clusterStep.Ck.copy_(Ck1)

    logger.info(f"Clustering ended in {MAX_ITER} iterations out of {MAX_ITER}")
    logger.info(f"Last diff {last_diff}")
    if start_clusters is not None:
        nEmptyClusters = (nItemsClusters < 1).sum().item()
        logger.info(f"{nEmptyClusters} empty clusters out of {k}")
    return clusterStep.Ck


def fastDPMean(dataLoader, featureMaker, l, MAX_ITER=100, batchSize=1000, EPSILON=1e-4, perIterSize=-1, save_dir=None,
               save_last=5, mu_start=None):
    """clustering.py:208-329: the distance is the norm, sqrt of the kernel's min_sq; one host decision per batch
    (maxDist > l), as the reference's own synchronisation."""
    logging.basicConfig(level=logging.INFO)
    logger = logging.getLogger("DPMean")
    logger.setLevel(logging.INFO)          # (basicConfig does nothing when the root logger already has a handler)
    save = save_dir is not None
    if save:
        save_dir = Path(save_dir)
        logger.addHandler(setup_log_file(save_dir))

    logger.info(f"{perIterSize} updates per iteration")
    device = _device()

    with torch.no_grad():
        if mu_start is not None:
            mu = mu_start.clone().to(device)
            _, k, D = mu.size()
        else:
            print("Start training from scratch. Creating new mu ...")
            mu = 0
            nSeqs = 100
            for index, data in enumerate(dataLoader):
                features = featureMaker(data)
                mu += features
                if index > nSeqs:
                    break

            B, S, D = mu.size()
            k = 1
            mu = mu.contiguous().view(-1, D).mean(dim=0).view(1, k, D)
            mu /= nSeqs

        def resetTmpData():
            mu1 = torch.zeros(mu.size(), device=device)
            c1 = torch.zeros(mu.size(1), dtype=torch.long, device=device)
            return mu1, c1

        mu1, c1 = resetTmpData()

        iter = 0
        while iter < MAX_ITER:
            start_time = time()
            for nBatch, data in enumerate(dataLoader):
                features = featureMaker(data)
                N, S, _ = features.size()
                features = features.contiguous().view(N * S, D)
                index, min_sq = kmeans_assign(features, mu)
                distance = min_sq.sqrt()
                maxDist = distance.max()

                if maxDist > l:
                    indexFeature = distance.argmax()
                    mu = torch.cat([mu, features[indexFeature].view(1, 1, D)], dim=1)
                    mu1 = torch.cat([mu1, torch.zeros(1, 1, D, device=mu.device)], dim=1)
                    c1 = torch.cat([c1, torch.zeros(1, device=mu.device, dtype=torch.long)], dim=0)
                    index[indexFeature] = k
                    k += 1
                    if k % 10 == 0:
                        logger.info(f"Number of clusters increased to {k}")

                kmeans_accumulate(features, index, mu1, c1)

            c1 = c1.float().view(1, -1, 1) + 1e-4
            mu1 /= c1
            last_diff = (mu - mu1).norm(dim=2).max().item()
            nItems = int(c1.sum().cpu().detach().item())

            mu = mu1
            k = mu.size(1)
            mu1, c1 = resetTmpData()

            iter += 1
            print()

            logger.info(
                f"ITER {iter} done in {time()-start_time:.2f} seconds. nItems: {nItems}. lambda={l}. mu shape: {mu.size()}. Difference with last checkpoint: {last_diff}"
            )

            if save:
                _save_step(save_dir, iter, save_last, mu, last_diff, "DPMean", logger)

            if last_diff < EPSILON:
                logger.info(f"Clustering ended in {iter} iterations out of {MAX_ITER}")
                break

    _, k, D = mu.size()
    logger.info(f"{k} clusters found for lambda = {l}")
    return mu


def KMean(C, k, MAX_ITER=100, EPSILON=1e-4, batchSize=1000):
    """clustering.py:332-358 on the rows C [N, D] (on the GPU); an empty cluster's mean is NaN, as in the reference."""
    _lib.require_gpu(C)
    N, D = C.size()
    indexes = torch.randperm(N)[:k]
    Ck = C[indexes.to(C.device)].view(1, k, D)

    with torch.no_grad():
        for iter in range(MAX_ITER):
            index, _ = kmeans_assign(C, Ck, want_min_sq=False)
            sums = torch.zeros(1, k, D, device=C.device)
            counts = torch.zeros(k, dtype=torch.long, device=C.device)
            kmeans_accumulate(C, index, sums, counts)
            Ck1 = sums / counts.float().view(1, -1, 1)
            last_diff = (Ck - Ck1).norm(dim=2).max().item()
            if last_diff < EPSILON:
                print(f"Clustering ended in {iter} iterations out of {MAX_ITER}")
                break
            Ck = Ck1

    print(f"Clustering ended in {MAX_ITER} iterations out of {MAX_ITER}")
    print(f"Last diff {last_diff}")
    return Ck


def distanceEstimation(featureMaker, dataLoader, maxIndex=10, maxSizeGroup=300):
    raise NotImplementedError("distanceEstimation (--getDistanceEstimation) is not on the MI355X path")
