"""cpc/criterion/seq_alignment.py of the reference on the device: collapseLabelChain (:62-84, cpc_probe_collapse), the CTC
prefix beam search (:11-61, cpc_ctc_beam_search), the Needleman-Wunsch alignment score and the phone error rate built on it
(:89-117, cpc_align_score), and getPER (:120-163).  Names and signatures are the reference's; the *_batch forms work on device
tensors and are what everything else calls.

The search does the reference's float32 arithmetic operation for operation, so wherever no two candidates of a frame score the
same its output equals the reference's bit for bit.  Deviation: EQUAL scores are ordered by (rank of the extended prefix in
the previous frame's beam, symbol) -- a prefix that is not extended counts as its own rank with symbol = blank -- where the
reference compares the prefixes' decimal strings.  The order is a function of the inputs alone (two runs give the same bytes),
and the search reports per sequence whether any frame met a tie among its first nKeep + 1 candidates.  A sequence whose scores
underflow to exactly 0 becomes all ties, as in the reference.
"""
import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, require_gpu, stream_ptr


def collapse_padded(inputLabels):
    """[N, T] frame labels -> (targets int64 [N, T], sizes int64 [N]): consecutive repeats removed, zero padded to T.  Nothing
    comes to the host (the CTC kernel takes the padded width as it is)."""
    require_gpu(inputLabels)
    labels = inputLabels.to(torch.int64).contiguous()
    n, t = labels.shape
    out = torch.empty(n, t, dtype=torch.int64, device=labels.device)
    sizes = torch.empty(n, dtype=torch.int64, device=labels.device)
    check(_lib.load().cpc_probe_collapse(ptr(labels), n, t, ptr(out), t, ptr(sizes), stream_ptr(labels.device)), "probe_collapse")
    return out, sizes


def collapseLabelChain(inputLabels):
    """(paddedOutput int64 [N, maxS], outSizes int64 [N]) with maxS the batch's largest collapsed length, as the reference
    returns it (one small copy to the host for maxS)."""
    out, sizes = collapse_padded(inputLabels)
    maxSize = int(sizes.max().item())
    return out[:, :maxSize].contiguous(), sizes


# --------------------------------------------------------------------------- CTC prefix beam search
def _refuse_without_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("cpc2_amd runs only on a GPU (HIP) device and none is available. There is no CPU fallback.")


def beam_search_batch(probs, lengths, nKeep, blankLabel, best_only=False):
    """probs [N, T, P] f32 probabilities on the device, lengths [N] (frames of row n to decode, 1 <= lengths[n] <= T; None: T
    everywhere) -> (scores f32 [N, R], sizes int32 [N, R], labels int32 [N, R, T], counts int32 [N], ties int32 [N]) on the
    device, R = 1 with best_only (the best prefix only) else nKeep: the kept prefixes best first, labels padded with -1, counts
    the rows that hold a prefix (fewer than nKeep exist only in the first frames), ties whether a frame met equal scores among
    its first nKeep + 1 candidates.  Rows of probs beyond lengths[n] are never read.  Nothing comes to the host."""
    if probs.dim() != 3:
        raise ValueError(f"beam_search_batch: probs must be [N, T, P] (got {tuple(probs.shape)})")
    n, t, p = probs.shape
    if t == 0 or n == 0:
        raise ValueError(f"beam_search_batch: nothing to decode (N = {n}, T = {t})")
    nKeep, blankLabel = int(nKeep), int(blankLabel)
    lib = _lib.load()
    nbytes = lib.cpc_ctc_beam_search_scratch_bytes(n, t, p, nKeep)
    if nbytes == 0:
        raise ValueError("beam_search_batch: " + lib.cpc_last_error().decode(errors="replace"))
    if not 0 <= blankLabel < p:
        raise ValueError(f"beam_search_batch: blankLabel={blankLabel} is outside [0, P={p})")
    require_gpu(probs, lengths)
    probs = _lib.f32c(probs)
    dev = probs.device
    if lengths is None:
        lengths = torch.full((n,), t, dtype=torch.int32, device=dev)
    lengths = lengths.to(torch.int32).contiguous()
    if lengths.shape != (n,):
        raise ValueError(f"beam_search_batch: lengths must be [N = {n}] (got {tuple(lengths.shape)})")
    rows = 1 if best_only else nKeep
    scores = torch.empty(n, rows, dtype=torch.float32, device=dev)
    sizes = torch.empty(n, rows, dtype=torch.int32, device=dev)
    labels = torch.empty(n, rows, t, dtype=torch.int32, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    ties = torch.empty(n, dtype=torch.int32, device=dev)
    buf = _lib.scratch(nbytes, dev)
    check(lib.cpc_ctc_beam_search(ptr(probs), ptr(lengths), n, t, p, nKeep, blankLabel, int(bool(best_only)), ptr(scores),
                                  ptr(sizes), ptr(labels), ptr(counts), ptr(ties), ptr(buf), buf.numel(), stream_ptr(dev)),
          "ctc_beam_search")
    return scores, sizes, labels, counts, ties


def beam_search(score_preds, nKeep, blankLabel):
    """The reference's beam_search: one [T, P] array (copied to the current device) or device tensor of probabilities ->
    [(score numpy.float32, [labels])] best first, at most nKeep of them."""
    if isinstance(score_preds, torch.Tensor):
        probs = score_preds
    else:
        probs = torch.from_numpy(np.ascontiguousarray(score_preds, dtype=np.float32))
    if probs.dim() != 2:
        raise ValueError(f"beam_search: score_preds must be [T, P] (got {tuple(probs.shape)})")
    if probs.shape[0] == 0:
        raise ValueError("beam_search: no frame to decode (T = 0)")
    if not isinstance(score_preds, torch.Tensor):
        _refuse_without_gpu()
        probs = probs.cuda()
    scores, sizes, labels, counts, _ = beam_search_batch(probs.float().unsqueeze(0), None, nKeep, blankLabel)
    scores, sizes, labels = scores[0].cpu().numpy(), sizes[0].cpu().numpy(), labels[0].cpu().numpy()
    return [(scores[i], [int(x) for x in labels[i, :sizes[i]]]) for i in range(int(counts[0]))]


# --------------------------------------------------------------------------- alignment score and phone error rate
def align_score_batch(seq1, len1, seq2, len2, d, m, r):
    """NeedlemanWunschAlignScore without its normalisation for n pairs: seq1 [n, L1], seq2 [n, L2] padded integer matrices and
    their lengths [n] on the device -> int32 [n] on the device (integers: exact)."""
    require_gpu(seq1, len1, seq2, len2)
    n = seq1.shape[0]
    if n == 0 or seq2.shape[0] != n or len1.shape != (n,) or len2.shape != (n,):
        raise ValueError(f"align_score_batch: {n} rows of seq1 against {seq2.shape[0]} of seq2, lengths {tuple(len1.shape)} and "
                         f"{tuple(len2.shape)}")
    dev = seq1.device

    def matrix(x):
        x = x.to(torch.int32)
        return x.contiguous() if x.shape[1] > 0 else torch.zeros(n, 1, dtype=torch.int32, device=dev)

    a, b = matrix(seq1), matrix(seq2)
    la = len1.to(torch.int32).clamp(max=seq1.shape[1]).contiguous()
    lb = len2.to(torch.int32).clamp(max=seq2.shape[1]).contiguous()
    out = torch.empty(n, dtype=torch.int32, device=dev)
    check(_lib.load().cpc_align_score(ptr(a), a.shape[1], ptr(la), ptr(b), b.shape[1], ptr(lb), n, int(d), int(m), int(r), ptr(out),
                                      stream_ptr(dev)), "align_score")
    return out


def get_seq_PER_batch(seqLabels, sizes, detectedLabels, detectedSizes):
    """get_seq_PER of n pairs on the device: float64 [n] = (substitutions + insertions + deletions) / sizes (inf or nan where
    sizes is 0, where the reference raises)."""
    return align_score_batch(seqLabels, sizes, detectedLabels, detectedSizes, -1, -1, 0).double() / sizes.double()


def _as_row(seq):
    _refuse_without_gpu()
    if isinstance(seq, torch.Tensor):
        require_gpu(seq)
        row = seq.reshape(1, -1)
    else:
        row = torch.tensor([int(x) for x in seq], dtype=torch.int32).reshape(1, -1).cuda()
    return row, torch.tensor([row.shape[1]], dtype=torch.int32, device=row.device)


def NeedlemanWunschAlignScore(seq1, seq2, d, m, r, normalize=True):
    """The reference's function on one pair (lists, arrays or device tensors of labels)."""
    if normalize and len(seq1) == 0:
        raise ZeroDivisionError("float division by zero")
    a, la = _as_row(seq1)
    b, lb = _as_row(seq2)
    res = int(align_score_batch(a, la, b.to(a.device), lb.to(a.device), d, m, r).item())
    if normalize:
        res /= float(len(seq1))
    return res


def get_seq_PER(seqLabels, detectedLabels):
    return NeedlemanWunschAlignScore(seqLabels, detectedLabels, -1, -1, 0,
                                     normalize=True)


def window_PER(dataLoader, featureMaker, blankLabel, nKeep=100):
    """(per-window PER float64 [windows], per-window tie flag bool [windows]) as numpy arrays: getPER before its mean.  Per batch
    one launch of the search (best prefix only), one of the score, and one copy to the host: the windows' scores and flags."""
    pers, tied = [], []
    for data in dataLoader:
        with torch.no_grad():
            probs = featureMaker(data)
        labels, sizes = collapse_padded(data[1].to(probs.device))
        _, found_sizes, found, _, ties = beam_search_batch(probs, None, nKeep, blankLabel, best_only=True)
        per = get_seq_PER_batch(labels, sizes, found[:, 0], found_sizes[:, 0])
        host = torch.stack([per, ties.double()]).cpu().numpy()
        pers.append(host[0])
        tied.append(host[1] != 0)
    if not pers:
        return np.zeros(0), np.zeros(0, bool)
    return np.concatenate(pers), np.concatenate(tied)


def getPER(dataLoader, featureMaker, blankLabel, nKeep=100):
    """The reference's getPER: the mean over all windows of get_seq_PER(collapsed frame labels, best prefix of the beam search
    over featureMaker(data), an [N, S, P] tensor of probabilities on the device); data[1] are the frame labels.  No process per
    window; the windows' values are summed in float64 in loader order (the reference sums them in a shared C float in the order
    its processes finish)."""
    pers, _ = window_PER(dataLoader, featureMaker, blankLabel, nKeep)
    return mean_std(pers)[0]


def mean_std(values):
    """(mean, standard deviation) of the windows' values, summed in order in float64: avgPER and sqrt(varPER) of the reference's
    cpc/eval/common_voices_eval.py:340-351."""
    out, squares = 0, 0
    for value in values:
        out += float(value)
        squares += float(value) * float(value)
    mean = out / len(values)
    return mean, max(squares / len(values) - mean ** 2, 0.0) ** 0.5
