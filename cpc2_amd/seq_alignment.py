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

CTC forced alignment (ctc_forced_align, frame_labels; csrc/ctc_align.hip, include/cpc2_hip.h version 120) is NOT the reference's:
it has no aligner, so the definition is the specification.  One sequence has logits x [T][k] (float32), targets y[0..L) and
blank = k - 1; extended states s in [0, 2 L + 1), sym(s) = blank for even s and y[s // 2] for odd s.  Every alignment emits one
symbol per frame, so sum_t lse_t is common to all paths and the maximisation runs on the raw logits:
    start  v[0][0] = x[0][blank]; v[0][1] = x[0][y0] when L >= 1; every other state -inf
    step   v[t][s] = max(v[t-1][s], v[t-1][s-1] when s >= 1, v[t-1][s-2] when s is odd, s >= 3 and y[s//2] != y[s//2 - 1])
                     + x[t][sym(s)], all float64, the max first, then ONE addition (a host statement with the same operation
           order gives the same bits)
    ties   among equal finite candidates s wins over s - 1, which wins over s - 2; at the end state 2 L wins over 2 L - 1 unless
           the latter is strictly larger.  ties = 1 when a maximum on the returned path, the end included, had an equal finite
           competitor
    status 0 aligned; 1 no alignment exists (T < L + #{i: y[i] == y[i-1]}, or T = 0); 2 an argument of that sequence is invalid
           (input length outside [0, t_max], target length outside [0, max_l], a label outside [0, k - 1)).  With 1 or 2 the
           path is -1 on every frame, the scores are NaN and first / last / confidence are -1 / -1 / NaN.
Agreement with torchaudio.functional.forced_align is UNMEASURED (torchaudio is not a dependency and was not at hand).
"""
from collections import namedtuple

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
    """probs [N, T, P] f32 probabilities on the device, lengths [N] (frames of row n to decode; None: T everywhere) -> (scores
    f32 [N, R], sizes int32 [N, R], labels int32 [N, R, T], counts int32 [N], ties int32 [N]) on the device, R = 1 with
    best_only (the best prefix only) else nKeep: the kept prefixes best first, labels padded with -1, counts the rows that hold
    a prefix (fewer than nKeep exist only in the first frames), ties whether a frame met equal scores among its first nKeep + 1
    candidates.  lengths[n] is clamped to [0, T]: a length above T decodes the T frames there are, and a length of 0 or below
    decodes nothing -- that row returns the empty prefix alone, with score 1.0, counts 1 and ties 0.  Rows of probs beyond
    lengths[n] are never read.  Nothing comes to the host."""
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


# --------------------------------------------------------------------------- CTC forced alignment
MAX_ALIGN_TARGET = 1024        # cpc_ctc_align: labels per utterance (the extended states live in LDS)

AlignResult = namedtuple("AlignResult", ["path", "labels", "score", "log_prob", "status", "ties", "first", "last", "confidence"])
AlignResult.__doc__ = """ctc_forced_align's result, all on the device, b sequences of up to t_max frames and max_l labels:
path int32 [b, t_max] (the state per frame, -1 from the input length on), labels int64 [b, t_max] (the path mapped through sym:
a target label, the blank k - 1, or -1 where the path is -1), score float64 [b] (the path's logit sum), log_prob float64 [b]
(score - sum_t lse_t: the path's log posterior), status int32 [b], ties int32 [b], first / last int32 [b, max_l] (the first and
last frame of every token, -1 beyond the target length) and confidence float32 [b, max_l] (the mean log posterior of the token's
label over its frames)."""


def ctc_forced_align(logits, in_lengths, targets, tgt_lengths):
    """The best CTC alignment (module docstring) of logits [b, t_max, k] float32 (blank = k - 1) with int64 device tables
    in_lengths [b], targets [b, W], tgt_lengths [b] -> AlignResult.  Rows of logits at or beyond an input length and target padding
    are never read.  Targets wider than the kernel holds (min(t_max, 1024) labels) are cut to that width: a sequence whose target
    length lies beyond it then has status 2.  Two launches, no float atomic, and no copy to the host: the caller synchronises when
    it reads the result."""
    if logits.dim() != 3 or targets.dim() != 2:
        raise ValueError(f"ctc_forced_align: logits must be [b, t_max, k] and targets [b, W] (got {tuple(logits.shape)} and "
                         f"{tuple(targets.shape)})")
    require_gpu(logits, in_lengths, targets, tgt_lengths)
    lib = _lib.load()
    logits = _lib.f32c(logits)
    b, t, k = logits.shape
    dev = logits.device
    if in_lengths.shape != (b,) or tgt_lengths.shape != (b,) or targets.shape[0] != b:
        raise ValueError(f"ctc_forced_align: {b} sequences, but in_lengths {tuple(in_lengths.shape)}, targets {tuple(targets.shape)}, "
                         f"tgt_lengths {tuple(tgt_lengths.shape)}")
    max_l = min(targets.shape[1], t, MAX_ALIGN_TARGET)
    nbytes = lib.cpc_ctc_align_scratch_bytes(b, t, max_l)
    if nbytes == 0:
        raise ValueError("ctc_forced_align: " + lib.cpc_last_error().decode(errors="replace"))
    in_lengths = in_lengths.to(torch.int64).contiguous()
    tgt_lengths = tgt_lengths.to(torch.int64).contiguous()
    targets = targets[:, :max_l].to(torch.int64).contiguous()
    path = torch.empty(b, t, dtype=torch.int32, device=dev)
    score = torch.empty(b, 2, dtype=torch.float64, device=dev)
    status = torch.empty(b, dtype=torch.int32, device=dev)
    ties = torch.empty(b, dtype=torch.int32, device=dev)
    lse = torch.empty(b, t, dtype=torch.float64, device=dev)
    first = torch.empty(b, max_l, dtype=torch.int32, device=dev)
    last = torch.empty(b, max_l, dtype=torch.int32, device=dev)
    conf = torch.empty(b, max_l, dtype=torch.float32, device=dev)
    buf = _lib.scratch(nbytes, dev)
    tg = ptr(targets) if max_l else None
    check(lib.cpc_ctc_align(ptr(logits), b, t, k, ptr(in_lengths), tg, max_l, ptr(tgt_lengths), ptr(path), ptr(score), ptr(status),
                            ptr(ties), ptr(lse), ptr(buf), buf.numel(), stream_ptr(dev)), "ctc_align")
    if max_l:
        check(lib.cpc_ctc_align_segments(ptr(logits), b, t, k, tg, max_l, ptr(tgt_lengths), ptr(path), ptr(status), ptr(lse), ptr(first),
                                         ptr(last), ptr(conf), stream_ptr(dev)), "ctc_align_segments")
    blank = torch.full_like(path, k - 1, dtype=torch.int64)
    if max_l:
        token = targets.gather(1, (path.clamp(min=0) >> 1).clamp(max=max_l - 1).to(torch.int64))
        labels = torch.where((path & 1) == 1, token, blank)
    else:
        labels = blank
    labels = torch.where(path < 0, torch.full_like(labels, -1), labels)
    return AlignResult(path, labels, score[:, 0], score[:, 1], status, ties, first, last, conf)


def _host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def head_frame_of(n_frames, n_head, kernel=8, stride=4):
    """For each of n_frames feature frames the head frame whose receptive-field centre is nearest:
    j = clamp((f - (kernel - stride) // 2) // stride, 0, n_head - 1); (f - 2) // 4 for the default head."""
    f = np.arange(int(n_frames), dtype=np.int64)
    return np.clip((f - (kernel - stride) // 2) // stride, 0, max(int(n_head) - 1, 0))


def head_tokens(path_row):
    """The token index of every head frame of one path (numpy, -1 padded): a frame in state 2 i + 1 has token i, a blank frame the
    preceding token, leading blanks the first token.  None when the path holds no token (L = 0 or no alignment)."""
    path_row = np.asarray(path_row)
    states = path_row[path_row >= 0]
    if len(states) == 0 or states[-1] == 0:
        return None
    return np.maximum((states.astype(np.int64) - 1) // 2, 0)


def frame_labels(result, n_frames, kernel=8, stride=4, blank_label=None):
    """One label per 10 ms feature frame for every sequence of an AlignResult (or anything with `path` and `labels`, tensors or
    arrays [b, t_max]): n_frames [b] feature frames each -> a list of int64 arrays, None for a sequence without frame labels.
    Feature frame f takes head frame j = clamp((f - (kernel - stride) // 2) // stride, 0, T - 1), T = the frames of the path.
    Blank head frames take the preceding token's label and leading blanks the first token's; with blank_label given they take
    that id instead.  A sequence with status 1 or 2 has none, nor has one with L = 0 unless blank_label is given.  The tensors
    come to the host here (hand over host arrays to copy once for several uses)."""
    path, labels = _host(result.path), _host(result.labels)
    out = []
    for row in range(path.shape[0]):
        states = path[row][path[row] >= 0]
        n_head = len(states)
        if n_head == 0:
            out.append(None)
            continue
        lab = labels[row, :n_head].astype(np.int64)
        if blank_label is not None:
            head = np.where(states & 1, lab, int(blank_label))
        else:
            tokens = head_tokens(states)
            if tokens is None:
                out.append(None)
                continue
            token_label = np.zeros(int(tokens.max()) + 1, np.int64)
            odd = (states & 1) == 1
            token_label[(states[odd] - 1) // 2] = lab[odd]
            head = token_label[tokens]
        out.append(head[head_frame_of(int(n_frames[row]), n_head, kernel, stride)])
    return out


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
