"""PCA and linear slow-feature analysis (SFA) of a model's features -- cpc/criterion/research/dim_reduction.py of the reference:
the same names, constructor arguments, registered buffers and state-dict keys, so a file written by either side loads in the other
(DESIGN.md section 20).

    python -m cpc2_amd.dim_reduction CKPT.pt OUT.pt --pathDB AUDIO_DIR [--seqList F] [--recursionLevel 2] [--extension .flac]
           [--mode SFA|PCA] [--debug] [--batchSize 8] [--sizeWindow 20480] [--exact_counts]

What is built differently:

    update    accumulates on the device in f64 -- PCA through cpc2_amd.cca.Moments (cpc_moments_accumulate, one stream), SFALinear
              through cpc_seq_moments_accumulate with skip = 1: the sums, the products of the frames and the products of the
              frame-to-frame differences inside each window in one pass, no [N, k, k] broadcast and no difference tensor.  The f64
              totals live beside the f32 buffers and are not part of the state dict.
    build     runs on the host in numpy float64 from those totals (centring, the per-dimension standard deviation, a Cholesky
              factor and its inverse, eigh) and fills the f32 buffers once at the end.  Eigenvalues ascend as torch.symeig gave
              them.  LAPACK leaves an eigenvector's sign open; here (a deviation) each one is signed so that its component of
              largest magnitude is positive, the first such index winning.
    forward   never touches its input (the reference subtracts the mean in the caller's tensor): cpc_center_scale_rows, then ONE
              cpc_gemm_nt with the folded matrix -- PCA_mul[0], or for SFA projection[0] @ normalizer[0] formed in f64, rounded to
              f32 once and kept until selectDimensions or a load changes it.

Host tensors are refused: there is no CPU fallback.
"""
import argparse
import json
import os
import sys
from random import shuffle

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, require_gpu, scratch, stream_ptr
from .cca import Moments, _rows

MAX_DIM = 512            # cpc_seq_moments_accumulate, cpc_center_scale_rows


def _sign_rows(rows):
    """Each row times the sign of its component of largest magnitude (the first such index)."""
    pick = np.argmax(np.abs(rows), axis=1)
    sign = np.sign(rows[np.arange(rows.shape[0]), pick])
    sign[sign == 0.0] = 1.0
    return rows * sign[:, None]


def _fill(module, name, array):
    """Registered buffer `name` <- a float64 host array, rounded to the buffer's dtype once, on the buffer's device."""
    old = getattr(module, name)
    setattr(module, name, torch.from_numpy(np.ascontiguousarray(array)).to(device=old.device, dtype=old.dtype))


def _project(x, k, mean, scale, weight):
    """((x - mean) / (scale + 1e-8)) @ weight^T on the device for x [n, k] or [b, s, k]; x is left as it was."""
    require_gpu(x)
    x2, ld, n = _rows(x, k, "x")
    m = weight.shape[0]
    out = torch.empty(n, m, dtype=torch.float32, device=x.device)
    if n:
        lib = _lib.load()
        centred = torch.empty(n, k, dtype=torch.float32, device=x.device)
        check(lib.cpc_center_scale_rows(ptr(x2), ld, ptr(mean), ptr(scale), ptr(centred), k, n, k, stream_ptr(x.device)),
              "center_scale_rows")
        check(lib.cpc_gemm_nt(ptr(centred), k, ptr(weight), k, ptr(out), m, None, n, m, k, stream_ptr(x.device)), "gemm_nt")
    return out.view(*x.shape[:-1], m)


def _save(dimRed, kind, path):
    """{"state_dict", "inDim", "type"}: the file of the reference's command line."""
    torch.save({"state_dict": dimRed.state_dict(), "inDim": dimRed.k, "type": kind}, path)


class PCA(torch.nn.Module):
    """dim_reduction.py:13-62.  update([n, k] or [b, s, k]) accumulates, build() solves, forward projects onto every component
    (rows of PCA_mul[0], eigenvalues ascending)."""

    def __init__(self, k):
        super(PCA, self).__init__()
        if not 1 <= k <= MAX_DIM:
            raise ValueError(f"PCA: k={k} outside the supported limits (1 <= k <= {MAX_DIM})")
        self.building = True
        self.register_buffer('var', torch.zeros(k, k))
        self.register_buffer('mean', torch.zeros(k))
        self.register_buffer('PCA_mul', torch.zeros(1, k, k))
        self.register_buffer('PCA_values', torch.zeros(k))
        self.N = 0
        self.k = k
        self.moments = None          # cca.Moments: the f64 totals, on the device of the first update

    def update(self, x):
        require_gpu(x)
        if self.moments is None:
            self.moments = Moments(self.k, device=x.device)
        before = self.moments.count
        with torch.no_grad():
            self.moments.update(x)
        self.N += self.moments.count - before

    def totals(self):
        """(sum x [k], sum x x^T [k, k]) as host float64 arrays."""
        if self.moments is None:
            raise RuntimeError("PCA: no update has run")
        _, sx, _, sxx, _, _ = self.moments.state()
        return sx, sxx

    def build(self, normalize=True):
        self.normalize = normalize               # (stored and never read, as in the reference)
        sx, sxx = self.totals()
        mean = sx / self.N
        var = sxx / self.N - mean[None, :] * mean[:, None]
        vals, vecs = np.linalg.eigh(var)
        # the float64 solution stays beside the buffers (not in the state dict), which hold it rounded to f32 once
        self.solution = dict(var=var, mean=mean, PCA_mul=_sign_rows(vecs.T)[None], PCA_values=vals)
        for name, value in self.solution.items():
            _fill(self, name, value)
        self.building = False

    def forward(self, x):
        assert(not self.building)
        return _project(x, self.k, self.mean, None, self.PCA_mul[0])

    def save(self, path):
        _save(self, "PCA", path)


class SFALinear(torch.nn.Module):
    """dim_reduction.py:65-148: whitening of the features followed by the eigenvectors of the whitened covariance of their
    frame-to-frame differences; the slowest directions come first (eigenvalues ascending).

    Counts.  The reference's update drops frame 0 of every window [N, S, k], then sums S - 1 frames and S - 2 differences per
    window, but adds N * S to N_x and N * (S - 1) to N_speed: 3 windows of 16 frames give N_x = 48 for 45 summed rows and
    N_speed = 45 for 42 differences.  Its mean_x is therefore (S - 1) / S of the mean of the summed frames, and on features with an
    offset the whitening is visibly wrong at short windows (the covariance of the output is 0.65 to 0.99 away from the identity
    at S = 16 .. 64; at S = 128 the factor is 127 / 128).  Those counts are the default here, so that a fit on the same data gives the
    reference's numbers.  exact_counts=True divides by the rows and differences actually summed: mean_x is then S / (S - 1) times
    the default's when every window has S frames."""

    def __init__(self, k, exact_counts=False):
        super(SFALinear, self).__init__()
        if not 1 <= k <= MAX_DIM:
            raise ValueError(f"SFALinear: k={k} outside the supported limits (1 <= k <= {MAX_DIM})")
        self.register_buffer('covar_speed', torch.zeros(k, k))
        self.register_buffer('mean_x', torch.zeros(k))
        self.register_buffer('square_x', torch.zeros(k))
        self.register_buffer('covar_x', torch.zeros(k, k))
        self.register_buffer('normalizer', torch.zeros(1, k, k))
        self.register_buffer('PCA_mul', torch.zeros(1, k, k))
        self.register_buffer('PCA_values', torch.zeros(k))
        self.register_buffer('projection', torch.zeros(1, k, k))
        self.N_speed = 0
        self.N_x = 0
        self.rows_summed = 0
        self.differences_summed = 0
        self.exact_counts = exact_counts
        self.k = k
        self.building = True
        self.sums = self.gram = self.dgram = None      # the f64 totals, on the device of the first update
        self._folded = None

    def update(self, x):
        require_gpu(x)
        if x.dtype != torch.float32:
            raise TypeError(f"cpc2_amd kernels are fp32 only (got {x.dtype})")
        if x.dim() != 3 or x.size(2) != self.k:
            raise ValueError(f"SFALinear.update: expected [N, S, {self.k}], got {tuple(x.shape)}")
        N, S, k = x.size()
        if N == 0:
            return
        if S < 2:
            raise ValueError(f"SFALinear.update: windows of {S} frame(s); frame 0 is dropped, so at least 2 are required")
        if not (x.stride(2) == 1 and x.stride(1) >= k and x.stride(0) >= S * x.stride(1)):
            x = x.contiguous()
        if self.sums is None:
            self.sums = torch.zeros(k, dtype=torch.float64, device=x.device)
            self.gram = torch.zeros(k, k, dtype=torch.float64, device=x.device)
            self.dgram = torch.zeros(k, k, dtype=torch.float64, device=x.device)
        lib = _lib.load()
        nb = lib.cpc_seq_moments_scratch_bytes(N, S, 1, k)
        check(lib.cpc_seq_moments_accumulate(ptr(x), x.stride(1), x.stride(0), N, S, 1, k, ptr(self.sums), ptr(self.gram),
                                             ptr(self.dgram), ptr(scratch(nb, x.device)), nb, stream_ptr(x.device)),
              "seq_moments_accumulate")
        self.N_speed += N * (S - 1)
        self.N_x += N * S
        self.rows_summed += N * (S - 1)
        self.differences_summed += N * (S - 2)

    def totals(self):
        """(sum x [k], sum x x^T [k, k], sum dx dx^T [k, k]) over the kept frames, as host float64 arrays."""
        if self.sums is None:
            raise RuntimeError("SFALinear: no update has run")
        return self.sums.cpu().numpy(), self.gram.cpu().numpy(), self.dgram.cpu().numpy()

    def build(self):
        sums, gram, dgram = self.totals()
        n_x, n_speed = (self.rows_summed, self.differences_summed) if self.exact_counts else (self.N_x, self.N_speed)
        if self.differences_summed < 1:
            raise ValueError("SFALinear.build: no frame-to-frame difference was summed (windows of 2 frames)")
        mean = sums / n_x
        covar = gram / n_x - mean[None, :] * mean[:, None]
        # standard deviation of each dimension
        square = np.sqrt(np.clip(np.diag(gram) / n_x - mean * mean, 0.0, None))
        inv_square = 1.0 / (square + 1e-08)
        # inverse Cholesky factor of the covariance of the normalized features: l l^T = covar_normalized
        covar_normalized = inv_square[:, None] * covar * inv_square[None, :]
        l_ = np.linalg.inv(np.linalg.cholesky(covar_normalized))
        # covariance of the differences, in the whitened coordinates
        speed = inv_square[:, None] * (dgram / n_speed) * inv_square[None, :]
        speed = l_ @ (speed @ l_.T)
        vals, vecs = np.linalg.eigh(speed)
        mul = _sign_rows(vecs.T)[None]
        # the float64 solution stays beside the buffers (not in the state dict), which hold it rounded to f32 once
        self.solution = dict(covar_speed=speed, mean_x=mean, square_x=square, covar_x=covar, normalizer=l_[None], PCA_mul=mul,
                             PCA_values=vals, projection=mul)
        for name, value in self.solution.items():
            _fill(self, name, value)
        self._folded = None
        self.building = False

    def selectDimensions(self, indexVector):
        self.projection = self.PCA_mul[0, indexVector > 0].view(1, -1, self.k)
        self._folded = None

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # a file saved behind selectDimensions holds a projection of fewer rows
        saved = state_dict.get(prefix + "projection")
        if saved is not None and saved.dim() == 3 and saved.shape[2] == self.k and saved.shape != self.projection.shape:
            self.projection = self.projection.new_zeros(saved.shape)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        self._folded = None

    def folded(self):
        """projection[0] @ normalizer[0] [rows kept, k], formed in f64 and rounded to f32 once."""
        if self._folded is None or self._folded.device != self.projection.device:
            both = self.projection[0].cpu().double().numpy() @ self.normalizer[0].cpu().double().numpy()
            self._folded = torch.from_numpy(both.astype(np.float32)).to(self.projection.device)
        return self._folded

    def forward(self, x):
        assert(not self.building)
        return _project(x, self.k, self.mean_x, self.square_x, self.folded())

    def save(self, path):
        _save(self, "SFA", path)


def _fit(dimRed, dataLoader, featureMaker):
    ar = getattr(getattr(featureMaker, "featureMaker", None), "gAR", None)
    with torch.no_grad():
        for data in dataLoader:
            hidden = getattr(ar, "hidden", None)
            if hidden is not None:                   # a carried state fits one batch size: a shorter last batch starts afresh
                held = hidden[0] if isinstance(hidden, tuple) else hidden
                if held.size(1) != data[0].size(0):
                    ar.hidden = None
            dimRed.update(featureMaker(data))
    return dimRed


def buildPCA(dataLoader, featureMaker, k, normalize=False):
    output_PCA = PCA(k)
    output_PCA.cuda()
    print("Performing the PCA...")
    _fit(output_PCA, dataLoader, featureMaker)
    output_PCA.build(normalize=normalize)
    return output_PCA


def buildSFA(dataLoader, featureMaker, k, exact_counts=False):
    output_SFA = SFALinear(k, exact_counts=exact_counts)
    output_SFA.cuda()
    featureMaker.collapse = False
    print("Performing the SFA...")
    _fit(output_SFA, dataLoader, featureMaker)
    output_SFA.build()
    return output_SFA


def loadDimReduction(path, centroidLimits):
    state_dict = torch.load(path, map_location="cpu")
    if state_dict["type"] == "PCA":
        if centroidLimits is not None:
            raise ValueError(f"{path} holds a PCA, which has no selectDimensions: centroidLimits applies to an SFA only")
        dimRed = PCA(state_dict["inDim"])
    elif state_dict["type"] == "SFA":
        dimRed = SFALinear(state_dict["inDim"])
    else:
        raise ValueError(f"Invalid module type {state_dict['type']}")
    if centroidLimits is not None and "centroid_values" not in state_dict:
        raise ValueError(f"{path} has no 'centroid_values' (no tool writes one; add a [k] tensor under that key to the file): "
                         "centroidLimits cannot select dimensions")
    dimRed.load_state_dict(state_dict["state_dict"])
    dimRed.building = False
    if centroidLimits is not None:
        centroidsVals = state_dict["centroid_values"]
        dimRed.selectDimensions((centroidsVals > centroidLimits[0]) * (centroidsVals < centroidLimits[1]))
    return dimRed


class ModelDimReduced(torch.nn.Module):
    """A feature maker followed by a fitted PCA / SFALinear, as one module: what buildFeature*, buildAllFeature and kMeanGPU take
    where they take a FeatureModule or a ModelClusterCombined."""

    def __init__(self, featureMaker, dimRed):
        super(ModelDimReduced, self).__init__()
        self.model = featureMaker
        self.dimRed = dimRed

    @property
    def out_feature_dim(self):
        return (self.dimRed.projection if isinstance(self.dimRed, SFALinear) else self.dimRed.PCA_mul).size(1)

    def getDownsamplingFactor(self):
        return self.model.getDownsamplingFactor()

    def forward(self, data):
        return self.dimRed(self.model(data))


# --------------------------------------------------------------------------- the command line
def parseArgs(argv):
    parser = argparse.ArgumentParser(description='Dim reduction. Performing either a PCA or a SFA')
    parser.add_argument('pathCheckpoint', type=str)
    parser.add_argument('pathOut', type=str)
    parser.add_argument('--pathDB', type=str, required=True)
    parser.add_argument('--seqList', type=str, default=None)
    parser.add_argument('--recursionLevel', type=int, default=2)
    parser.add_argument('--extension', type=str, default='.flac')
    parser.add_argument('--mode', type=str, default='SFA', choices=['PCA', 'SFA'])
    parser.add_argument('--debug', action='store_true')
    parser.add_argument('--batchSize', type=int, default=8)
    parser.add_argument('--sizeWindow', type=int, default=20480)
    parser.add_argument('--exact_counts', action='store_true',
                        help="SFA: divide by the rows and differences actually summed, not by the reference's counts")
    return parser.parse_args(argv)


def refuse_unsupported(args):
    if args.extension.lower() == ".mp3":
        raise SystemExit("--extension .mp3: there is no mp3 decoder in this package; convert the files to .wav or .flac")
    if not (args.pathCheckpoint.endswith(".pt") and os.path.isfile(args.pathCheckpoint)):
        raise SystemExit(f"pathCheckpoint {args.pathCheckpoint}: not an existing .pt checkpoint")
    if os.path.exists(args.pathOut):
        raise SystemExit(f"pathOut {args.pathOut} exists: the tool overwrites nothing")
    if args.batchSize < 1 or args.sizeWindow < 1:
        raise SystemExit(f"--batchSize {args.batchSize} --sizeWindow {args.sizeWindow}: at least 1 each")


def main(argv, timings=None):
    import time
    from . import dataset as ds
    from .feature_loader import FeatureModule, loadModel

    args = parseArgs(argv)
    refuse_unsupported(args)
    timings = {} if timings is None else timings
    t0 = time.perf_counter()
    seqNames, speakers = ds.findAllSeqs(args.pathDB, speaker_level=args.recursionLevel, extension=args.extension)
    if args.seqList is not None:
        seqNames = ds.filterSeqs(args.seqList, seqNames)
    if args.debug:
        shuffle(seqNames)
        seqNames = seqNames[:100]
    dataset = ds.AudioBatchData(args.pathDB, args.sizeWindow, seqNames, None, len(speakers))
    trainLoader = dataset.getDataLoader(args.batchSize, "sequential", False, numWorkers=0)
    t1 = time.perf_counter()
    timings["load"] = t1 - t0

    model, outDim, _ = loadModel([args.pathCheckpoint])
    model.gAR.keepHidden = True
    featureMaker = FeatureModule(model, False).cuda()
    featureMaker.eval()
    if args.mode == 'SFA':
        dim_reduction = buildSFA(trainLoader, featureMaker, outDim, exact_counts=args.exact_counts)
    else:
        dim_reduction = buildPCA(trainLoader, featureMaker, outDim)
    t2 = time.perf_counter()
    timings["fit"] = t2 - t1

    dim_reduction.save(args.pathOut)
    pathArgs = f"{os.path.splitext(args.pathOut)[0]}_args.json"
    with open(pathArgs, 'w') as file:
        json.dump(vars(args), file, indent=2)
    timings["write"] = time.perf_counter() - t2
    return dim_reduction


if __name__ == "__main__":
    main(sys.argv[1:])
