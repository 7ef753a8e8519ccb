"""CTC forced alignment on the GPU (csrc/ctc_align.hip through the C ABI, seq_alignment.ctc_forced_align,
CTCphone_criterion.align and `common_voices_eval align`) against the float64 statement of tests/ctc_align_oracle.py.

path, status, ties, score[0], first and last are compared BY EQUALITY, tied cases included: the tie rule is part of the
definition.  score[1], lse and conf are held to the first-order bounds that the statement's docstring derives (2 ulp ASSUMED for
the device's f64 exp and log); the worst ratio against the bound is printed.  Every launch writes into buffers with poisoned
guard zones on both sides, rows of the logits at or beyond an input length are NaN and target padding is out of range."""
import json
import os

import numpy as np
import pytest
import torch

import ctc_align_oracle as oracle
from cpc2_amd import _lib, audio
from cpc2_amd.dataset import parseSeqLabels
from cpc2_amd.eval import common_voices_eval as cv
from cpc2_amd.seq_alignment import AlignResult, ctc_forced_align

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DB = os.path.join(GOLDEN, "test_db")
TRANSCRIPTS = os.path.join(GOLDEN, "g27_phone_transcripts.txt")
SEQ_LIST = os.path.join(GOLDEN, "seq_list.txt")
CHECKPOINT = os.path.join(GOLDEN, "ref_checkpoint", "checkpoint_7.pt")
DEV = "cuda:0"
GUARD = 64
WORKGROUP = 256                  # ctc_align.hip: CA_THREADS, the stride of the threads over the states


def _p(t):
    return _lib.ptr(t)


def _st():
    return _lib.stream_ptr(torch.device(DEV))


def _dev(a, dtype=None):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


class _Guarded:
    """A device buffer of `shape` between two guard zones of a value the kernels never write."""

    def __init__(self, shape, dtype, poison):
        n = int(np.prod(shape))
        self.whole = torch.full((n + 2 * GUARD,), poison, dtype=dtype, device=DEV)
        self.view = self.whole[GUARD:GUARD + n].view(*shape)
        self.poison, self.n = poison, n

    def intact(self):
        edge = torch.cat([self.whole[:GUARD], self.whole[GUARD + self.n:]])
        return bool((edge == self.poison).all())

    def numpy(self):
        return self.view.cpu().numpy()


def _launch(logits, in_len, targets, tgt_len, scratch_byte=0x5a, want_lse=True):
    """cpc_ctc_align + cpc_ctc_align_segments through the C ABI -> dict of numpy outputs.  Rows of the logits at or beyond each
    (valid) input length are NaN, target padding is out of range, every output has poisoned guards, the scratch is filled with
    `scratch_byte`."""
    lib = _lib.load()
    logits = np.array(logits, np.float32)
    targets = np.array(targets, np.int64).reshape(len(logits), -1)
    b, t_max, k = logits.shape
    max_l = targets.shape[1]
    for i in range(b):
        if 0 <= in_len[i] <= t_max:
            logits[i, int(in_len[i]):] = np.nan
        if 0 <= tgt_len[i] <= max_l:
            targets[i, int(tgt_len[i]):] = 10 ** 9
    lg, il, tg, tl = _dev(logits), _dev(in_len, torch.int64), _dev(targets), _dev(tgt_len, torch.int64)
    out = dict(path=_Guarded((b, t_max), torch.int32, 77), score=_Guarded((b, 2), torch.float64, 7.5),
               status=_Guarded((b,), torch.int32, 77), ties=_Guarded((b,), torch.int32, 77),
               lse=_Guarded((b, t_max), torch.float64, 7.5), first=_Guarded((b, max(max_l, 1)), torch.int32, 77),
               last=_Guarded((b, max(max_l, 1)), torch.int32, 77), conf=_Guarded((b, max(max_l, 1)), torch.float32, 7.5))
    nb = lib.cpc_ctc_align_scratch_bytes(b, t_max, max_l)
    assert nb > 0
    scratch = _Guarded((nb,), torch.uint8, scratch_byte)
    scratch.whole[:GUARD] = 0xa5
    scratch.whole[GUARD + nb:] = 0xa5
    tgp = _p(tg) if max_l else None
    _lib.check(lib.cpc_ctc_align(_p(lg), b, t_max, k, _p(il), tgp, max_l, _p(tl), _p(out["path"].view), _p(out["score"].view),
                                 _p(out["status"].view), _p(out["ties"].view), _p(out["lse"].view) if want_lse else None,
                                 _p(scratch.view), nb, _st()), "ctc_align")
    if want_lse:
        _lib.check(lib.cpc_ctc_align_segments(_p(lg), b, t_max, k, tgp, max_l, _p(tl), _p(out["path"].view), _p(out["status"].view),
                                              _p(out["lse"].view), _p(out["first"].view), _p(out["last"].view), _p(out["conf"].view),
                                              _st()), "ctc_align_segments")
    torch.cuda.synchronize()
    for name, buf in out.items():
        assert buf.intact(), f"{name}: written outside its buffer"
    edge = torch.cat([scratch.whole[:GUARD], scratch.whole[GUARD + nb:]])
    assert bool((edge == 0xa5).all()), "scratch: written outside its buffer"
    res = {name: buf.numpy() for name, buf in out.items()}
    if max_l == 0:
        res["first"], res["last"], res["conf"] = (res[n][:, :0] for n in ("first", "last", "conf"))
    return res


def _compare(got, refs, what, segments=True):
    """Equality of what the definition fixes, the bounds for what passes through exp and log; returns the worst ratio."""
    worst = 0.0
    for i, ref in enumerate(refs):
        tag = f"{what} sequence {i}"
        assert got["status"][i] == ref["status"], tag
        assert got["ties"][i] == ref["ties"], tag
        assert np.array_equal(got["path"][i], ref["path"]), tag
        if ref["status"] != 0:
            assert np.isnan(got["score"][i]).all() and np.isnan(got["lse"][i]).all(), tag
            if segments:
                assert (got["first"][i] == -1).all() and (got["last"][i] == -1).all() and np.isnan(got["conf"][i]).all(), tag
            continue
        assert got["score"][i, 0] == ref["score"][0], tag                            # the same additions in the same order
        n = int((ref["path"] >= 0).sum())
        assert np.isnan(got["lse"][i, n:]).all(), tag
        ratios = [abs(got["score"][i, 1] - ref["score"][1]) / ref["b_score1"]]
        ratios += list(np.abs(got["lse"][i, :n] - ref["lse"][:n]) / ref["b_lse"][:n])
        if segments:
            assert np.array_equal(got["first"][i], ref["first"]) and np.array_equal(got["last"][i], ref["last"]), tag
            n_lab = int((ref["first"] >= 0).sum())
            assert np.isnan(got["conf"][i, n_lab:]).all(), tag
            ratios += list(np.abs(got["conf"][i, :n_lab].astype(np.float64) - ref["conf"][:n_lab].astype(np.float64)) /
                           ref["b_conf"][:n_lab])
        assert np.isfinite(ratios).all() and max(ratios) <= 1.0, (tag, max(ratios))
        worst = max(worst, max(ratios))
    print(f"{what}: worst error / bound of score[1], lse and conf = {worst:.3f}")
    return worst


def _check(logits, in_len, targets, tgt_len, what):
    got = _launch(logits, in_len, targets, tgt_len)
    refs = oracle.align_batch(logits, in_len, targets, tgt_len)
    _compare(got, refs, what)
    return got, refs


def _targets(rng, b, max_l, k, repeats=True):
    y = rng.integers(0, k - 1, (b, max(max_l, 1)))[:, :max_l]
    if repeats and max_l >= 4 and k > 2:
        y[:, 1] = y[:, 0]                                    # a repeated label: the skip move is barred there
    return y.astype(np.int64)


# ----------------------------------------------------------------------------- edges, and the range of k
@pytest.mark.parametrize("k", [2, 5, 300])
def test_edges(k):
    """L = 0; T = L = 1; T = L (the forced diagonal); y = [a, a] with T = 2 (no alignment) and T = 3; T = 0; a target with one
    frame fewer than its repeats need."""
    rng = np.random.default_rng(k)
    t_max, max_l = 7, 5
    logits = (rng.standard_normal((8, t_max, k)) * 2).astype(np.float32)
    a = 0
    diag = list(range(min(5, k - 1))) if k > 2 else [0]                 # k = 2 has one label: its diagonal is T = L = 1
    rows = [(6, []), (1, [a]), (len(diag), diag), (2, [a, a]), (3, [a, a]), (0, [a]), (0, []), (4, [a, a, a])]
    targets = np.zeros((8, max_l), np.int64)
    for i, (_, y) in enumerate(rows):
        targets[i, :len(y)] = y
    in_len, tgt_len = [r[0] for r in rows], [len(r[1]) for r in rows]
    got, refs = _check(logits, in_len, targets, tgt_len, f"edges k={k}")
    assert [r["status"] for r in refs] == [0, 0, 0, 1, 0, 1, 1, 1]
    assert list(got["path"][0]) == [0] * 6 + [-1] and list(got["path"][1][:2]) == [1, -1]
    assert list(got["path"][2][:len(diag)]) == [2 * i + 1 for i in range(len(diag))]
    assert list(got["path"][4][:3]) == [1, 2, 3] and got["ties"][4] == 0


def test_batch_of_three_with_poison_around_everything():
    """Input lengths t_max, 1 and a middle value, target lengths 0, 1 and max_l; NaN rows behind each input length, out-of-range
    ids in the target padding, guards around every output and the scratch; the same without the optional lse."""
    rng = np.random.default_rng(3)
    t_max, max_l, k = 37, 9, 6
    logits = (rng.standard_normal((3, t_max, k)) * 2).astype(np.float32)
    targets = _targets(rng, 3, max_l, k)
    in_len, tgt_len = [t_max, 1, 20], [0, 1, max_l]
    got, refs = _check(logits, in_len, targets, tgt_len, "batch of three")
    assert [r["status"] for r in refs] == [0, 0, 0]
    bare = _launch(logits, in_len, targets, tgt_len, want_lse=False)
    for name in ("path", "score", "status", "ties"):
        assert np.array_equal(bare[name], got[name], equal_nan=True), name
    assert (bare["lse"] == 7.5).all()                                    # not given: not written


# ----------------------------------------------------------------------------- state counts around the workgroup size
@pytest.mark.parametrize("n_lab", [WORKGROUP // 2 - 1, WORKGROUP // 2, WORKGROUP // 2 + 22, 3 * WORKGROUP // 2 - 1, 3 * WORKGROUP // 2])
def test_state_counts_around_the_workgroup_size(n_lab):
    """2 L + 1 = 255 and 257 (odd: just below and just above the workgroup's 256 threads), 301 (no multiple), 767 and 769 (the
    third stride); per case one sequence with exactly the frames its target needs (the band is one path wide at both ends), one
    with frames to spare and one shorter target."""
    rng = np.random.default_rng(n_lab)
    k = 11
    targets = _targets(rng, 3, n_lab, k)
    need = oracle.needed_frames(targets[0])
    t_max = need + 70
    logits = (rng.standard_normal((3, t_max, k)) * 2).astype(np.float32)
    in_len, tgt_len = [need, t_max, t_max - 33], [n_lab, n_lab, n_lab - 5]
    _, refs = _check(logits, in_len, targets, tgt_len, f"2L+1={2 * n_lab + 1}")
    assert [r["status"] for r in refs] == [0, 0, 0] and 2 * n_lab + 1 in (255, 257, 301, 767, 769)


def test_at_the_limit():
    """b = 2, t_max = 4096, max_l = 1024: every frame and every state the kernel holds, and 8.4 MB of back-pointers a sequence."""
    rng = np.random.default_rng(4096)
    t_max, max_l, k = 4096, 1024, 5
    logits = (rng.standard_normal((2, t_max, k)) * 2).astype(np.float32)
    targets = _targets(rng, 2, max_l, k)
    _, refs = _check(logits, [t_max, 3001], targets, [max_l, 700], "the limit")
    assert [r["status"] for r in refs] == [0, 0]


# ----------------------------------------------------------------------------- ties
def test_all_zero_logits_tie_wherever_a_frame_is_spare():
    t_max, max_l, k = 40, 12, 4
    logits = np.zeros((5, t_max, k), np.float32)
    targets = np.array([[0, 1, 2] * 4, [0, 0, 1, 1] * 3, [2] * 12, [1, 0] * 6, [0] * 12], np.int64)
    in_len, tgt_len = [40, 40, 23, 12, 9], [12, 12, 12, 12, 0]
    got, refs = _check(logits, in_len, targets, tgt_len, "all-zero logits")
    needs = [oracle.needed_frames(targets[i, :tgt_len[i]]) for i in range(5)]
    assert needs == [12, 18, 23, 12, 0]
    # L >= 1 and a frame to spare: a tie; no frame to spare (rows 2 and 3): one path only; L = 0: one path only
    assert list(got["ties"]) == [1, 1, 0, 0, 0]


def test_small_integer_logits_meet_ties_everywhere_and_agree():
    """Logits in {0, 1, 2}: equal candidates at many cells, on and off the best path.  The returned path is the tie rule's."""
    rng = np.random.default_rng(8)
    t_max, max_l, k = 90, 20, 5
    logits = rng.integers(0, 3, (6, t_max, k)).astype(np.float32)
    targets = _targets(rng, 6, max_l, k)
    got, refs = _check(logits, [90, 61, 45, 33, 25, 90], targets, [20, 20, 17, 9, 20, 1], "integer logits")
    assert sum(r["ties"] for r in refs) >= 3 and all(r["status"] == 0 for r in refs)


def test_random_logits_with_positive_margins_have_no_tie():
    rng = np.random.default_rng(9)
    t_max, max_l, k = 120, 30, 41
    logits = (rng.standard_normal((4, t_max, k)) * 3).astype(np.float32)
    targets = _targets(rng, 4, max_l, k)
    got, refs = _check(logits, [120, 77, 64, 35], targets, [30, 30, 11, 30], "random logits")
    assert all(r["status"] == 0 and r["ties"] == 0 for r in refs) and (got["ties"] == 0).all()


# ----------------------------------------------------------------------------- invalid sequences, determinism, refusals
@pytest.mark.parametrize("what", ["input length", "negative input length", "target length", "label", "negative label"])
def test_an_invalid_sequence_has_status_2_and_leaves_the_others_alone(what):
    rng = np.random.default_rng(11)
    t_max, max_l, k = 30, 8, 6
    logits = (rng.standard_normal((4, t_max, k)) * 2).astype(np.float32)
    targets = _targets(rng, 4, max_l, k)
    in_len, tgt_len = [30, 22, 17, 9], [8, 5, 8, 3]
    good = _launch(logits, in_len, targets, tgt_len)
    if what == "input length":
        in_len[1] = t_max + 1
    elif what == "negative input length":
        in_len[1] = -1
    elif what == "target length":
        tgt_len[1] = max_l + 1
    elif what == "label":
        targets[1, 2] = k - 1                                           # the blank is no label
    else:
        targets[1, 0] = -1
    got, refs = _check(logits, in_len, targets, tgt_len, what)
    assert [r["status"] for r in refs] == [0, 2, 0, 0] and list(got["status"]) == [0, 2, 0, 0]
    keep = [0, 2, 3]
    for name in got:
        assert np.array_equal(got[name][keep], good[name][keep], equal_nan=True), name


def test_two_launches_into_differently_poisoned_scratch_give_the_same_bytes():
    rng = np.random.default_rng(12)
    t_max, max_l, k = 300, 140, 7
    logits = rng.integers(0, 4, (3, t_max, k)).astype(np.float32) + (rng.standard_normal((3, t_max, k)) * 0.5).astype(np.float32) * (
        rng.random((3, t_max, 1)) < 0.5)                                # half of the frames tie-prone
    targets = _targets(rng, 3, max_l, k)
    in_len, tgt_len = [300, 171, 299], [140, 100, 0]
    first = _launch(logits, in_len, targets, tgt_len, scratch_byte=0x00)
    second = _launch(logits, in_len, targets, tgt_len, scratch_byte=0xff)
    for name in first:
        assert first[name].tobytes() == second[name].tobytes(), name
    _compare(first, oracle.align_batch(logits, in_len, targets, tgt_len), "determinism case")


def test_refusals():
    lib = _lib.load()
    t_max, max_l, k = 12, 4, 5
    lg = torch.zeros(1, t_max, k, device=DEV)
    il, tl = _dev([t_max], torch.int64), _dev([max_l], torch.int64)
    tg = torch.zeros(1, max_l, dtype=torch.int64, device=DEV)
    path, score = torch.zeros(1, t_max, dtype=torch.int32, device=DEV), torch.zeros(1, 2, dtype=torch.float64, device=DEV)
    status, ties = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    lse = torch.zeros(1, t_max, dtype=torch.float64, device=DEV)
    first, last = torch.zeros(1, max_l, dtype=torch.int32, device=DEV), torch.zeros(1, max_l, dtype=torch.int32, device=DEV)
    conf = torch.zeros(1, max_l, device=DEV)
    nb = lib.cpc_ctc_align_scratch_bytes(1, t_max, max_l)
    sc = torch.zeros(nb, dtype=torch.uint8, device=DEV)

    def align(b=1, t=t_max, kk=k, ml=max_l, scratch=sc, nbytes=nb):
        return lib.cpc_ctc_align(_p(lg), b, t, kk, _p(il), _p(tg), ml, _p(tl), _p(path), _p(score), _p(status), _p(ties), _p(lse),
                                 _p(scratch), nbytes, _st())

    def segments(b=1, t=t_max, kk=k, ml=max_l):
        return lib.cpc_ctc_align_segments(_p(lg), b, t, kk, _p(tg), ml, _p(tl), _p(path), _p(status), _p(lse), _p(first), _p(last),
                                          _p(conf), _st())

    assert align() == 0 and segments() == 0
    for bad in [dict(b=0), dict(b=65536), dict(t=0), dict(t=4097), dict(kk=1), dict(kk=65537), dict(ml=-1), dict(ml=t_max + 1),
                dict(t=4096, ml=1025)]:
        for call, name in ((align, b"ctc_align:"), (segments, b"ctc_align_segments:")):
            assert call(**bad) == -1, bad                                # CPC_ERR_INVALID
            assert lib.cpc_last_error().startswith(name) and b"supported limits" in lib.cpc_last_error(), bad
    assert align(nbytes=nb - 1) == -3 and b"scratch" in lib.cpc_last_error()          # CPC_ERR_WORKSPACE
    assert align(scratch=None, nbytes=nb) == -3
    assert lib.cpc_ctc_align(None, 1, t_max, k, _p(il), _p(tg), max_l, _p(tl), _p(path), _p(score), _p(status), _p(ties), None,
                             _p(sc), nb, _st()) == -1 and b"null buffer" in lib.cpc_last_error()
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- the Python entry point
def test_ctc_forced_align_returns_the_named_result():
    rng = np.random.default_rng(21)
    t_max, max_l, k = 50, 12, 9
    logits = (rng.standard_normal((4, t_max, k)) * 2).astype(np.float32)
    targets = _targets(rng, 4, max_l, k)
    in_len, tgt_len = [50, 31, 5, 40], [12, 7, 9, 0]                    # row 2 has no alignment
    res = ctc_forced_align(_dev(logits), _dev(in_len, torch.int64), _dev(targets), _dev(tgt_len, torch.int64))
    assert isinstance(res, AlignResult) and res._fields == ("path", "labels", "score", "log_prob", "status", "ties", "first", "last",
                                                            "confidence")
    assert all(t.is_cuda for t in res)
    refs = oracle.align_batch(logits, in_len, targets, tgt_len)
    got = dict(path=res.path.cpu().numpy(), score=torch.stack([res.score, res.log_prob], 1).cpu().numpy(),
               status=res.status.cpu().numpy(), ties=res.ties.cpu().numpy(), first=res.first.cpu().numpy(),
               last=res.last.cpu().numpy(), conf=res.confidence.cpu().numpy(), lse=np.full((4, t_max), np.nan))
    for i, ref in enumerate(refs):                                      # (lse is not part of the named result)
        got["lse"][i] = ref["lse"]
    _compare(got, refs, "ctc_forced_align")
    labels = res.labels.cpu().numpy()
    assert labels.dtype == np.int64
    for i, ref in enumerate(refs):
        assert np.array_equal(labels[i], oracle.labels_of(ref["path"], targets[i, :tgt_len[i]], k - 1)), i
        if ref["status"] == 0:
            assert oracle.collapse(labels[i, :in_len[i]], k - 1) == list(targets[i, :tgt_len[i]])
    assert [r["status"] for r in refs] == [0, 0, 1, 0] and (labels[2] == -1).all()
    # targets of width 0, wider targets than frames (cut to t_max), and CPU tensors
    none = ctc_forced_align(_dev(logits), _dev(in_len, torch.int64), torch.zeros(4, 0, dtype=torch.int64, device=DEV),
                            torch.zeros(4, dtype=torch.int64, device=DEV))
    assert none.first.shape == (4, 0) and (none.status.cpu().numpy() == 0).all()
    assert np.array_equal(none.labels.cpu().numpy(), np.where(np.arange(t_max)[None] < np.array(in_len)[:, None], k - 1, -1))
    wide = np.concatenate([targets, np.zeros((4, 60), np.int64)], axis=1)
    cut = ctc_forced_align(_dev(logits), _dev(in_len, torch.int64), _dev(wide), _dev(tgt_len, torch.int64))
    assert cut.first.shape == (4, t_max) and torch.equal(cut.path, res.path) and torch.equal(cut.first[:, :max_l], res.first)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ctc_forced_align(torch.zeros(1, 4, 3), torch.tensor([4]), torch.zeros(1, 1, dtype=torch.int64), torch.tensor([1]))
    with pytest.raises(ValueError, match="ctc_align: sizes outside the supported limits"):
        ctc_forced_align(torch.zeros(1, 4097, 3, device=DEV), _dev([4], torch.int64), _dev([[0]], torch.int64), _dev([1], torch.int64))


# ----------------------------------------------------------------------------- CTCphone_criterion.align
@pytest.mark.parametrize("lstm,seq_norm", [(False, False), (True, False), (False, True), (True, True)])
def test_criterion_align_equals_the_statement_on_getPrediction(lstm, seq_norm):
    torch.manual_seed(27)
    crit = cv.CTCphone_criterion(32, 5, LSTM=lstm, seqNorm=seq_norm, dropout=True).to(DEV)
    with torch.no_grad():
        for p in crit.PhoneCriterionClassifier.parameters():
            p.mul_(8.0)                                                  # logits a few units apart, as a trained head's
    crit.train()                                                         # align itself must switch to eval: dropout is on
    rng = np.random.default_rng(5)
    c = _dev(rng.standard_normal((3, 60, 32)).astype(np.float32))
    sizes = _dev([60, 41, 22], torch.int64)
    label = np.array([[1, 1, 3, 0, 4, 2], [4, 0, 0, 0, 0, 0], [2, 2, 0, 1, 0, 0]], np.int64)
    label_size = np.array([6, 1, 4], np.int64)
    res = crit.align(c, sizes, _dev(label), _dev(label_size))
    again = crit.align(c, sizes, _dev(label), _dev(label_size))
    assert crit.training and torch.equal(res.path, again.path) and not res.confidence.requires_grad
    crit.eval()
    with torch.no_grad():
        pred = crit.getPrediction(c, sizes)
    assert tuple(pred.shape) == (3, 14, 6)
    lengths = torch.clamp(sizes // crit.downsampling_factor, max=pred.size(1))            # perStep's
    assert lengths.tolist() == [14, 10, 5]
    assert (res.path >= 0).sum(1).tolist() == lengths.tolist()
    refs = oracle.align_batch(pred.cpu().numpy(), lengths.tolist(), label, label_size)
    assert [r["status"] for r in refs] == [0, 0, 0]
    got = dict(path=res.path.cpu().numpy(), score=torch.stack([res.score, res.log_prob], 1).cpu().numpy(),
               status=res.status.cpu().numpy(), ties=res.ties.cpu().numpy(), first=res.first.cpu().numpy(),
               last=res.last.cpu().numpy(), conf=res.confidence.cpu().numpy(), lse=np.stack([r["lse"] for r in refs]))
    _compare(got, refs, f"criterion LSTM={lstm} seqNorm={seq_norm}")


# ----------------------------------------------------------------------------- align, end to end
def test_align_end_to_end_on_a_one_epoch_run(tmp_path, capsys):
    run, align_dir = str(tmp_path / "run"), str(tmp_path / "aligned")
    cv.main(["train", DB, TRANSCRIPTS, CHECKPOINT, "--freeze", "--nEpochs", "1", "--batchSize", "4", "--pathVal", SEQ_LIST,
             "--file_extension", ".flac", "-o", run])
    names = [ln.strip() for ln in open(SEQ_LIST) if ln.strip()]
    assert len(names) == 7
    transcripts, n_phones = parseSeqLabels(TRANSCRIPTS)
    transcripts.pop("step")
    samples = {}
    for dirpath, _d, files in os.walk(DB):
        for f in files:
            if f.endswith(".flac") and f[:-5] in names:
                samples[f[:-5]] = audio.load(os.path.join(dirpath, f))[0].shape[-1]
    empty, impossible, too_long = names[0], names[1], names[2]
    frames_of = {n: min(samples[n] // 160 // 4, (max(samples.values()) // 160 - 8) // 4 + 1) for n in names}
    transcripts[empty] = []
    transcripts[impossible] = [1] * (frames_of[impossible] // 2 + 5)     # L <= T, but the repeats need 2 L - 1 > T frames
    transcripts[too_long] = [1, 2] * 1000                                # more labels than the batch has frames: invalid
    phone = str(tmp_path / "transcripts.txt")
    with open(phone, "w") as f:
        for n in names:
            f.write(" ".join([n] + [str(v) for v in transcripts[n]]) + "\n")
    blank = n_phones
    capsys.readouterr()
    log = cv.main(["align", run, "-o", align_dir, "--pathPhone", phone, "--pathVal", SEQ_LIST, "--batchSize", "3", "--blank_label",
                   str(blank), "--name", "t"])
    printed = capsys.readouterr().out
    assert open(os.path.join(run, "logs_align_t.txt")).read() == printed and "5 of 7 utterances aligned" in printed
    assert sorted(os.listdir(align_dir)) == ["alignment_frames.txt", "alignment_log.json", "alignment_segments.txt"]
    with open(os.path.join(align_dir, "alignment_log.json")) as f:
        written = json.load(f)
    assert written["utterances"] == 7 and written["aligned"] == 5 and written["no_alignment"] == [impossible]
    assert written["invalid"] == [too_long] and written["empty_transcription"] == [empty]
    assert 0 <= written["met_a_tie"] <= 5 and written["arguments"]["align_dir"] == align_dir and written["arguments"]["pathPhone"] == phone
    assert {k: written[k] for k in written if k not in ("seconds", "arguments")} == {k: log[k] for k in log if k not in ("seconds", "arguments")}

    parsed, _ = parseSeqLabels(os.path.join(align_dir, "alignment_frames.txt"))
    assert parsed.pop("step") == 160 and set(parsed) == set(names) - {impossible, too_long}
    segments = {}
    for ln in open(os.path.join(align_dir, "alignment_segments.txt")):
        name, label, start, end, conf = ln.split()
        segments.setdefault(name, []).append((int(label), float(start), float(end), float(conf), start, end))
    assert set(segments) == set(names) - {impossible, too_long, empty}
    for name, labels in parsed.items():
        assert len(labels) == samples[name] // 160, name                 # one label per 160 samples
        assert oracle.collapse(labels, blank) == transcripts[name], name            # the frame labels collapse to the transcription
        if name == empty:
            assert set(labels) == {blank}
            continue
        rows = segments[name]
        assert [r[0] for r in rows] == transcripts[name], name           # one segment per token, in order
        assert rows[0][4] == "0.000000" and abs(rows[-1][2] - samples[name] / 16000) <= 1e-6, name
        assert all(rows[i][5] == rows[i + 1][4] for i in range(len(rows) - 1)), name            # they tile [0, duration)
        assert all(r[2] > r[1] and r[3] <= 0 for r in rows), name
    # the files feed linear_separability --pathPhone: the frame labels without --blank_label are phones only
    with pytest.raises(ValueError, match="exists and is not empty"):
        cv.main(["align", run, "-o", align_dir])
    plain = str(tmp_path / "plain")
    cv.main(["align", run, "-o", plain, "--pathPhone", phone, "--pathVal", SEQ_LIST, "--batchSize", "7"])
    phones_only, _ = parseSeqLabels(os.path.join(plain, "alignment_frames.txt"))
    assert set(phones_only) == {"step"} | (set(names) - {impossible, too_long, empty})
    for name in set(phones_only) - {"step"}:
        merged = [a for a, b in zip(phones_only[name], [None] + phones_only[name][:-1]) if a != b]
        want = [a for a, b in zip(transcripts[name], [None] + transcripts[name][:-1]) if a != b]
        assert blank not in phones_only[name] and merged == want, name
        assert len(phones_only[name]) == samples[name] // 160
    assert open(os.path.join(plain, "alignment_segments.txt")).read() == open(os.path.join(align_dir, "alignment_segments.txt")).read()
