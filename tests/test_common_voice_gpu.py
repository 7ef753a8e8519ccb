"""Whole-utterance phone recognition on the GPU (csrc/ctc_head.hip through cpc2_amd/eval/common_voices_eval.py): every new entry
against the fp64 statements of tests/ctc_head_oracle.py at the smallest shapes that can still go wrong, CTCphone_criterion as a
whole against the reference's recorded getPrediction (tests/golden/g27_common_voice.npz) and the oracle, the utterance gather
against a host loop, and `train` followed by `per` on the nine utterances of tests/golden/test_db."""
import copy
import json
import math
import os
import random
import re

import numpy as np
import pytest
import torch

import ctc_head_oracle as oracle
from cpc2_amd import _lib
from cpc2_amd.dataset import findAllSeqs, parseSeqLabels
from cpc2_amd.eval import common_voices_eval as cv
from cpc2_amd.feature_loader import loadModel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DB = os.path.join(GOLDEN, "test_db")
TRANSCRIPTS = os.path.join(GOLDEN, "g27_phone_transcripts.txt")
SEQ_LIST = os.path.join(GOLDEN, "seq_list.txt")
CHECKPOINT = os.path.join(GOLDEN, "ref_checkpoint", "checkpoint_7.pt")
DEV = "cuda:0"
# alpha and beta are f64 (as in cpc_probe_ctc: tests/test_probe_gpu.py), so only the casts of the outputs and the f32 sum of the
# per-sequence losses round: far below the project's CTC bound
CTC_TOL = 2e-5


def _p(t):
    return _lib.ptr(t)


def _st():
    return _lib.stream_ptr(torch.device(DEV))


def _dev(a, dtype=None):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-300))


# ----------------------------------------------------------------------------- cpc_ctc_loss
T_MAX, B = 37, 6


def _ctc_case(k):
    """Input lengths: t_max, a shorter one, 1, 0, one frame fewer than the target needs, and (row 5) a target of length 0.
    Row 1 repeats labels."""
    rng = np.random.default_rng(100 + k)
    logits = (rng.standard_normal((B, T_MAX, k)) * 2).astype(np.float32)
    targets = rng.integers(0, k - 1, (B, 9))
    targets[1, :4] = [2, 2, 0, 0]
    targets[4, :3] = [1, 1, 3]                       # "1 1 3" needs 4 frames
    in_len = np.array([T_MAX, 20, 1, 0, 3, 30], np.int64)
    tgt_len = np.array([5, 4, 1, 2, 3, 0], np.int64)
    return logits, in_len, targets.astype(np.int64), tgt_len


def _ctc_run(logits, in_len, targets, tgt_len, reduction, grad=True, alias=False):
    lib = _lib.load()
    b, t, k = logits.shape
    lg, il, tg, tl = _dev(logits), _dev(in_len), _dev(targets), _dev(tgt_len)
    nll = torch.full((b,), 7.0, device=DEV)
    loss = torch.full((1,), 7.0, device=DEV)
    dl = (lg if alias else torch.full_like(lg, 7.0)) if grad else None
    nb = lib.cpc_ctc_loss_scratch_bytes(b, t, targets.shape[1])
    assert nb > 0
    sc = torch.empty(nb, dtype=torch.uint8, device=DEV)
    _lib.check(lib.cpc_ctc_loss(_p(lg), b, t, k, _p(il), _p(tg) if targets.shape[1] else None, targets.shape[1], _p(tl),
                                {"sum": 0, "mean": 1}[reduction], _p(nll), _p(loss), _p(dl), _p(sc), nb, _st()), "ctc_loss")
    return float(loss), nll.cpu().numpy(), None if dl is None else dl.cpu().numpy()


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("k", [6, 70])
def test_ctc_loss_vs_fp64(k, reduction):
    logits, in_len, targets, tgt_len = _ctc_case(k)
    ref_loss, ref_nll, ref_grad = oracle.ctc_len(logits, in_len, targets, tgt_len, reduction)
    assert ref_nll[3] == 0 and ref_nll[4] == 0 and (ref_nll[[0, 1, 2, 5]] > 0).all()       # rows 3 and 4 have no alignment
    loss, nll, grad = _ctc_run(logits, in_len, targets, tgt_len, reduction)
    print(f"k={k} {reduction}: loss {abs(loss - ref_loss) / abs(ref_loss):.2e} nll {np.abs(nll - ref_nll).max():.2e} "
          f"grad {_rel(grad, ref_grad):.2e}")
    assert abs(loss - ref_loss) <= CTC_TOL * abs(ref_loss)
    assert np.all(np.abs(nll - ref_nll) <= CTC_TOL * np.abs(ref_nll))
    assert np.abs(grad - ref_grad).max() <= CTC_TOL * np.abs(ref_grad).max()
    for row in range(B):                              # exactly 0 beyond each input length, and for the rows without an alignment
        assert (grad[row, in_len[row]:] == 0).all()
    assert nll[3] == 0 and nll[4] == 0 and (grad[3] == 0).all() and (grad[4] == 0).all()
    # identical bits on a second launch, without the gradient, and with the gradient written over the logits
    loss2, nll2, grad2 = _ctc_run(logits, in_len, targets, tgt_len, reduction)
    assert loss2 == loss and np.array_equal(nll2, nll) and np.array_equal(grad2, grad)
    loss3, nll3, _ = _ctc_run(logits, in_len, targets, tgt_len, reduction, grad=False)
    assert loss3 == loss and np.array_equal(nll3, nll)
    loss4, nll4, grad4 = _ctc_run(logits, in_len, targets, tgt_len, reduction, alias=True)
    assert loss4 == loss and np.array_equal(nll4, nll) and np.array_equal(grad4, grad)


def test_ctc_loss_never_reads_frames_beyond_the_input_length():
    logits, in_len, targets, tgt_len = _ctc_case(6)
    base = _ctc_run(logits, in_len, targets, tgt_len, "mean")
    poisoned = logits.copy()
    for row in range(B):
        poisoned[row, in_len[row]:] = np.nan
    got = _ctc_run(poisoned, in_len, targets, tgt_len, "mean")
    assert got[0] == base[0] and np.array_equal(got[1], base[1]) and np.array_equal(got[2], base[2])


@pytest.mark.parametrize("what", ["input length", "target length", "label"])
def test_ctc_loss_bad_rows_are_nan(what):
    logits, in_len, targets, tgt_len = _ctc_case(6)
    good = _ctc_run(logits, in_len, targets, tgt_len, "sum")
    if what == "input length":
        in_len[1] = T_MAX + 1
    elif what == "target length":
        tgt_len[1] = targets.shape[1] + 1
    else:
        targets[1, 2] = 5                             # the blank is no label
    loss, nll, grad = _ctc_run(logits, in_len, targets, tgt_len, "sum")
    assert math.isnan(loss) and math.isnan(nll[1]) and np.isnan(grad[1]).all()
    keep = [0, 2, 3, 4, 5]
    assert np.array_equal(nll[keep], good[1][keep]) and np.array_equal(grad[keep], good[2][keep])


def test_ctc_loss_padded_width_does_not_matter():
    logits, in_len, targets, tgt_len = _ctc_case(6)
    wide = _ctc_run(logits, in_len, targets, tgt_len, "mean")
    narrow = _ctc_run(logits, in_len, np.ascontiguousarray(targets[:, :5]), tgt_len, "mean")
    wider = _ctc_run(logits, in_len, np.concatenate([targets, np.full((B, 20), 99)], axis=1), tgt_len, "mean")
    for other in (narrow, wider):
        assert wide[0] == other[0] and np.array_equal(wide[1], other[1]) and np.array_equal(wide[2], other[2])


@pytest.mark.parametrize("k", [6, 70])
def test_ctc_loss_with_full_lengths_equals_probe_ctc_bit_for_bit(k):
    lib = _lib.load()
    logits, _, targets, tgt_len = _ctc_case(k)
    full = np.full(B, T_MAX, np.int64)
    loss, nll, grad = _ctc_run(logits, full, targets, tgt_len, "mean")
    lg, tg, tl = _dev(logits), _dev(targets), _dev(tgt_len)
    p_nll, p_loss, p_grad = torch.empty(B, device=DEV), torch.empty(1, device=DEV), torch.empty_like(lg)
    nb = lib.cpc_probe_ctc_scratch_bytes(B, T_MAX, targets.shape[1])
    sc = torch.empty(nb, dtype=torch.uint8, device=DEV)
    _lib.check(lib.cpc_probe_ctc(_p(lg), B, T_MAX, k, _p(tg), targets.shape[1], _p(tl), _p(p_nll), _p(p_loss), _p(p_grad), _p(sc), nb,
                                 _st()), "probe_ctc")
    assert loss == float(p_loss) and np.array_equal(nll, p_nll.cpu().numpy()) and np.array_equal(grad, p_grad.cpu().numpy())
    assert np.isfinite(grad).all() and (nll > 0).all()


# ----------------------------------------------------------------------------- normalisation over the first len frames
# Bounds.  Lengths 40 and 33: 2e-6 absolute, the augmentation tests' bound.  With len = 2 the frames beyond len reach |y| ~ 10^3
# and dx ~ 10^5, where 2e-6 absolute is far below one f32 ulp, so that utterance (and the others as well) is held element by
# element to the first-order f32 bound of the kernels.  The statistics are summed in f64, so with u = 2^-24:
#   y   = fl32(exact):                                              |err| <= u |y|
#   dx  = fl32(rstd32 (dy - [f < n] (A / n + B y32[f] / (n - 1)))),  B = sum_g dy[g] y32[g]:
#         |err[f]| <= u (2 |dx[f]| + [f < n] rstd |y[f]| / (n - 1) (|B| + sum_g |dy[g] y[g]|))
#         (the cast, rstd's rounding, y32[f]'s rounding, and the roundings of the y32[g] inside B).
# SLACK covers eps arriving as an f32 (1e-8 differs from float(1e-8) by 6e-9 relative) and the f64 sums; FLOOR an element that
# cancels to nothing.
SN_ABS = 2e-6
U = 2.0 ** -24
SLACK = 1e-8
FLOOR = 1e-12


@pytest.mark.parametrize("h", [32, 256])
def test_seqnorm_len_vs_fp64(h):
    lib = _lib.load()
    b, s, lengths = 3, 40, [40, 33, 2]
    rng = np.random.default_rng(h)
    x = (rng.standard_normal((b, s, h)) * (1 + np.arange(h) / h) + np.linspace(-2, 2, h)).astype(np.float32)
    dy = rng.standard_normal((b, s, h)).astype(np.float32)
    ref_y = oracle.seqnorm_len(x, lengths)
    ref_dx = oracle.seqnorm_len_backward(x, lengths, dy)
    xd, dyd, ln = _dev(x), _dev(dy), _dev(lengths, torch.int64)
    y, dx = torch.full_like(xd, 7.0), torch.full_like(xd, 7.0)
    mean, rstd = torch.empty(b, h, device=DEV), torch.empty(b, h, device=DEV)
    _lib.check(lib.cpc_seqnorm_len_forward(_p(xd), _p(ln), b, s, h, 1e-8, _p(y), _p(mean), _p(rstd), _st()), "seqnorm_len_forward")
    _lib.check(lib.cpc_seqnorm_len_backward(_p(dyd), _p(y), _p(rstd), _p(ln), b, s, h, _p(dx), _st()), "seqnorm_len_backward")
    y, dx, mean, rstd = y.cpu().numpy(), dx.cpu().numpy(), mean.double().cpu().numpy(), rstd.double().cpu().numpy()
    for i, n in enumerate(lengths):
        x64, dy64 = x[i].astype(np.float64), dy[i].astype(np.float64)
        m = x64[:n].mean(axis=0)
        r = 1.0 / np.sqrt(((x64[:n] - m) ** 2).sum(axis=0) / (n - 1) + 1e-8)
        assert np.abs((x64 - m) * r - ref_y[i]).max() <= 1e-12 * np.abs(ref_y[i]).max()         # (the oracle's own statistics)
        inside = (np.arange(s) < n)[:, None]
        big_b = (dy64 * ref_y[i]).sum(axis=0)
        bound_y = (U + SLACK) * np.abs(ref_y[i]) + FLOOR
        bound_dx = (U + SLACK) * (2 * np.abs(ref_dx[i]) + inside * r * np.abs(ref_y[i]) / (n - 1) *
                                  (np.abs(big_b) + np.abs(dy64 * ref_y[i]).sum(axis=0))) + FLOOR * np.abs(ref_dx[i]).max()
        ey, ex = np.abs(y[i] - ref_y[i]), np.abs(dx[i] - ref_dx[i])
        print(f"h={h} len={n}: y {ey.max():.2e} abs, {(ey / bound_y).max():.2f} of the bound (max |y| {np.abs(ref_y[i]).max():.1e}); "
              f"dx {ex.max():.2e} abs, {(ex / bound_dx).max():.2f} of the bound (max |dx| {np.abs(ref_dx[i]).max():.1e})")
        assert (ey <= bound_y).all() and (ex <= bound_dx).all()
        if n > 2:
            assert ey.max() <= SN_ABS and ex.max() <= SN_ABS
        # the saved statistics against the oracle's, and with them: frames at or beyond len are normalised like the others
        assert (np.abs(mean[i] - m) <= U * np.abs(m) + FLOOR).all()
        assert (np.abs(rstd[i] - r) <= (U + SLACK) * r).all()
        assert (np.abs(y[i, n:] - ((x64 - m) * r)[n:]) <= bound_y[n:]).all()
    # identical bits on a second launch
    y2 = torch.empty_like(xd)
    m2, r2 = torch.empty(b, h, device=DEV), torch.empty(b, h, device=DEV)
    _lib.check(lib.cpc_seqnorm_len_forward(_p(xd), _p(ln), b, s, h, 1e-8, _p(y2), _p(m2), _p(r2), _st()), "seqnorm_len_forward")
    assert np.array_equal(y2.cpu().numpy(), y)


def test_seqnorm_len_of_one_frame_and_bad_lengths_are_nan():
    lib = _lib.load()
    b, s, h = 4, 12, 32
    x = _dev(np.random.default_rng(0).standard_normal((b, s, h)).astype(np.float32))
    ln = _dev([12, 1, 0, 13], torch.int64)
    y, mean, rstd = torch.empty_like(x), torch.empty(b, h, device=DEV), torch.empty(b, h, device=DEV)
    _lib.check(lib.cpc_seqnorm_len_forward(_p(x), _p(ln), b, s, h, 1e-8, _p(y), _p(mean), _p(rstd), _st()), "seqnorm_len_forward")
    y = y.cpu().numpy()
    assert np.isfinite(y[0]).all() and np.isnan(y[1]).all() and np.isnan(y[2]).all() and np.isnan(y[3]).all()


# ----------------------------------------------------------------------------- the strided classifier
def _gemm_tol(k):
    return 2e-6 * max(1, k ** 0.5)          # tests/test_gpu_parity.py: test_gemm_nt / test_gemm_tn, k = the summed dimension


# h = 256 makes the product's K = ks h = 2048 with a handful of output tiles: the size at which cpc_gemm_nt splits K (the default CPC
# width), and the reason the forward goes through cpc_conv_head_forward, which lends the split room for an ordered sum
@pytest.mark.parametrize("h", [32, 256])
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("s", [40, 43])
def test_conv_head_vs_fp64(s, b, h):
    c, ks = 6, 8
    rng = np.random.default_rng(10 * s + b + h)
    x = rng.standard_normal((b, s, h)).astype(np.float32)
    w = (rng.standard_normal((c, h, ks)) / 16).astype(np.float32)
    bias = rng.standard_normal(c).astype(np.float32)
    p = (s - ks) // 4 + 1
    dout = rng.standard_normal((b, p, c)).astype(np.float32)
    ref = oracle.conv_head(x, w, bias)
    ref_dw, ref_db, ref_dx = oracle.conv_head_backward(x, w, dout)

    def run():
        xd, wd, bd = (_dev(a).requires_grad_() for a in (x, w, bias))
        out = cv._ConvHeadFn.apply(xd, wd, bd)
        assert tuple(out.shape) == (b, p, c)
        out.backward(_dev(dout))
        return dict(out=out.detach().cpu().numpy(), dW=wd.grad.cpu().numpy(), db=bd.grad.cpu().numpy(), dx=xd.grad.cpu().numpy())

    got = run()
    tols = dict(out=_gemm_tol(ks * h), dW=_gemm_tol(b * p), db=_gemm_tol(b * p), dx=_gemm_tol(2 * c))
    errs = dict(out=_rel(got["out"], ref), dW=_rel(got["dW"], ref_dw), db=_rel(got["db"], ref_db), dx=_rel(got["dx"], ref_dx))
    print(f"s={s} b={b} h={h}: " + " ".join(f"{k} {errs[k]:.2e}/{tols[k]:.1e}" for k in errs))
    for name in errs:
        assert errs[name] <= tols[name], name
    assert (got["dx"][:, 4 * (p + 1):] == 0).all()         # the frames left over belong to no output frame
    again = run()                                          # identical bits on a second launch, the K split included
    for name in got:
        assert np.array_equal(got[name], again[name]), name


def test_conv_head_refuses_fewer_frames_than_taps():
    xd, wd, bd = _dev(np.zeros((1, 7, 32), np.float32)), _dev(np.zeros((6, 32, 8), np.float32)), _dev(np.zeros(6, np.float32))
    with pytest.raises(ValueError, match="7 frames are fewer than the classifier's kernel size 8"):
        cv._ConvHeadFn.apply(xd, wd, bd)


# ----------------------------------------------------------------------------- CTCphone_criterion whole
def _g27_case(g, i):
    state = {k[len(f"gp{i}_p_"):]: g[k] for k in g.files if k.startswith(f"gp{i}_p_")}
    seq_norm, lstm = (bool(v) for v in g[f"gp{i}_flags"])
    return g[f"gp{i}_c"], g[f"gp{i}_sizes"], state, seq_norm, lstm, g[f"gp{i}_pred"]


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("i", range(4))
def test_criterion_vs_reference_and_fp64(golden, i, reduction):
    c, sizes, state, seq_norm, lstm, ref_pred = _g27_case(golden("g27_common_voice.npz"), i)
    crit = cv.CTCphone_criterion(32, 5, LSTM=lstm, seqNorm=seq_norm, reduction=reduction)
    crit.load_state_dict({k: torch.from_numpy(v).float() for k, v in state.items()})
    crit.to(DEV).eval()
    c32 = c.astype(np.float32)
    cd = _dev(c32).requires_grad_()
    sz = _dev(sizes)
    pred = crit.getPrediction(cd, sz)
    e_pred = _rel(pred.detach().cpu(), ref_pred)
    label = np.array([[1, 1, 3, 0], [4, 0, 0, 0], [2, 2, 0, 0]])
    label_size = np.array([3, 1, 2])
    ref = oracle.criterion(c32, sizes, {k: v.astype(np.float32) for k, v in state.items()}, seq_norm, lstm, label, label_size, reduction)
    loss = crit(cd, sz, _dev(label), _dev(label_size))
    assert tuple(loss.shape) == (1, 1)
    loss.mean().backward()
    e_loss = abs(float(loss.detach()) - ref["loss"]) / abs(ref["loss"])
    e_dc = _rel(cd.grad.cpu(), ref["dc"])
    used = [k for k in state if lstm or not k.startswith("conv1.")]
    e_par = {k: _rel(dict(crit.named_parameters())[k].grad.cpu(), ref["grads"][k]) for k in used}
    print(f"seqNorm={seq_norm} LSTM={lstm} {reduction}: pred {e_pred:.2e} loss {e_loss:.2e} dc {e_dc:.2e} " +
          " ".join(f"{k.split('.')[-1]} {e:.2e}" for k, e in e_par.items()))
    assert e_pred <= 1e-5
    assert ref["loss"] > 0 and e_loss <= CTC_TOL and e_dc <= CTC_TOL
    for k, e in e_par.items():
        assert e <= CTC_TOL, k
    if not lstm:
        assert all(p.grad is None for k, p in crit.named_parameters() if k.startswith("conv1."))


# ----------------------------------------------------------------------------- the utterance gather
def test_gather_utterances_equals_a_host_loop():
    rng = np.random.default_rng(1)
    pack = rng.standard_normal(1500).astype(np.float32)
    offsets = np.array([0, 300, 317, 900, 1400, 10], np.int64)
    lengths = np.array([300, 17, 513, 600, 200, 50], np.int64)       # item 4 leaves the pack: a row of zeros
    roffset = np.array([0, 5, 80, 600, 0, 51], np.int64)             # item 3 starts at its end; item 5's offset is beyond its length
    for max_len in (513, 100, 1):
        ref = np.zeros((6, max_len), np.float32)
        for i in range(6):
            if offsets[i] + lengths[i] <= len(pack) and roffset[i] <= lengths[i]:
                row = pack[offsets[i] + roffset[i]:offsets[i] + lengths[i]][:max_len]
                ref[i, :len(row)] = row
        out = cv.gather_utterances(_dev(pack), _dev(offsets), _dev(lengths), _dev(roffset), max_len)
        assert np.array_equal(out.cpu().numpy(), ref)
    out = cv.gather_utterances(_dev(pack), _dev(offsets[:2]), _dev(lengths[:2]), None, 300)
    assert np.array_equal(out[0].cpu().numpy(), pack[:300]) and np.array_equal(out[1, :17].cpu().numpy(), pack[300:317])
    assert (out[1, 17:] == 0).all()


@pytest.fixture(scope="module")
def nine():
    seqs, _ = findAllSeqs(DB, extension=".flac")
    labels, _ = parseSeqLabels(TRANSCRIPTS)
    return seqs, labels


def test_batches_equal_the_items(nine):
    seqs, labels = nine
    ds = cv.SingleSequenceDataset(DB, seqs, labels, random_offset_amplitude=80)
    loader = ds.batches(4, shuffle=False)
    assert len(loader) == 3
    random.seed(5)
    got = list(loader)
    assert [b[0].shape[0] for b in got] == [4, 4, 1] and all(isinstance(b, cv.UtteranceBatch) for b in got)
    random.seed(5)
    at = 0
    for seq, size_seq, phone, size_phone in got:
        assert seq.shape[1] == 1 and seq.shape[2] == int(size_seq.max()) and phone.shape[1] == ds.maxSizePhone
        for row in range(seq.shape[0]):
            item = ds[at]
            n = int(item[1])
            assert int(size_seq[row]) == n and int(size_phone[row]) == int(item[3])
            assert torch.equal(seq[row, 0, :n], item[0][0, :n]) and (seq[row, 0, n:] == 0).all()
            assert torch.equal(phone[row].cpu(), item[2])
            at += 1
    torch.manual_seed(3)
    first = [b[1].view(-1).tolist() for b in ds.batches(4, shuffle=True)]
    second = [b[1].view(-1).tolist() for b in ds.batches(4, shuffle=True)]
    assert len(sum(first, [])) == 9 and len(sum(second, [])) == 9


def test_get_per_equals_the_reference(golden):
    g = golden("g27_common_voice.npz")
    n = json.loads(str(g["meta"]))["n_per"]
    assert n == 3
    for i in range(n):
        size_pred, size_gt, blank = (int(v) for v in g[f"per{i}_args"])
        value = cv.get_per((torch.from_numpy(g[f"per{i}_pred"]).to(DEV), size_pred, torch.from_numpy(g[f"per{i}_gt"]), size_gt, blank))
        assert value == float(g[f"per{i}_value"])


# ----------------------------------------------------------------------------- train, then per
def test_train_then_per_on_the_nine_utterances(tmp_path, capsys, monkeypatch):
    out = str(tmp_path / "run")
    heads, batches, in_val = [], [], []
    val_step, prepare_data = cv.val_step, cv.prepare_data

    def recording_val_step(loader, model, criterion, factor):
        heads.append(copy.deepcopy(criterion.state_dict()))
        batches.append([])
        in_val.append(True)
        try:
            return val_step(loader, model, criterion, factor)
        finally:
            in_val.pop()

    def recording_prepare_data(data):
        res = prepare_data(data)
        if in_val:
            batches[-1].append(res)
        return res

    monkeypatch.setattr(cv, "val_step", recording_val_step)
    monkeypatch.setattr(cv, "prepare_data", recording_prepare_data)
    cv.main(["train", DB, TRANSCRIPTS, CHECKPOINT, "--freeze", "--nEpochs", "2", "--batchSize", "4", "--pathVal", SEQ_LIST,
             "--file_extension", ".flac", "-o", out])
    monkeypatch.undo()
    printed = capsys.readouterr().out
    with open(os.path.join(out, "args_training.json")) as f:
        args = json.load(f)
    assert args["pathVal"] == SEQ_LIST and args["freeze"] and args["loss_reduction"] == "mean" and args["file_extension"] == ".flac"
    state = torch.load(os.path.join(out, "checkpoint.pt"), "cpu")
    assert set(state) == {"classifier", "model", "bestLoss"}
    assert all(k.startswith("module.") for k in state["classifier"]) and all(k.startswith("module.") for k in state["model"])
    log = open(os.path.join(out, "logs_train.txt")).read()
    assert log == printed
    train_lines = re.findall(r"^Epoch (\d) loss train : (\S+)$", log, flags=re.M)
    val_lines = re.findall(r"^Epoch (\d) loss val : (\S+)$", log, flags=re.M)
    assert [e for e, _ in train_lines] == ["0", "1"] and [e for e, _ in val_lines] == ["0", "1"]
    values = [float(v) for _, v in train_lines + val_lines]
    assert all(math.isfinite(v) and v > 0 for v in values)
    assert state["bestLoss"] == min(float(v) for _, v in val_lines)

    # the first epoch's validation loss against the oracle: the same features, the head as it was at that validation pass
    assert len(heads) == 2 and [len(b) for b in batches] == [2, 2]
    model = loadModel([CHECKPOINT])[0]
    model.to(DEV).eval()
    head = {k: v.cpu().numpy() for k, v in heads[0].items()}
    total = 0.0
    for seq, size_seq, phone, size_phone in batches[0]:
        with torch.no_grad():
            c = model(seq, None)[0]
        total += oracle.criterion(c.cpu().numpy(), (size_seq // 160).cpu().numpy(), head, False, False, phone.cpu().numpy(),
                                  size_phone.cpu().numpy(), "mean")["loss"]
    ref_val = total / len(batches[0])
    got_val = float(val_lines[0][1])
    print(f"validation loss of epoch 0: {got_val} against the oracle's {ref_val}")
    assert abs(got_val - ref_val) <= 1e-4 * abs(ref_val)
    best = int(np.argmin([float(v) for _, v in val_lines]))
    for k, v in heads[best].items():
        assert torch.equal(state["classifier"]["module." + k], v.cpu())

    capsys.readouterr()
    mean = cv.main(["per", out, "--name", "t"])
    printed = capsys.readouterr().out
    assert open(os.path.join(out, "logs_per_t.txt")).read() == printed
    assert os.path.isfile(os.path.join(out, "args_validation_t.json"))
    avg = re.search(r"^Average PER (\S+)$", printed, flags=re.M)
    std = re.search(r"^Standard deviation PER (\S+)$", printed, flags=re.M)
    assert avg and std and math.isfinite(float(avg.group(1))) and math.isfinite(float(std.group(1)))
    assert float(avg.group(1)) == mean and float(avg.group(1)) > 0 and float(std.group(1)) >= 0
    assert re.search(r"^\d+ of 7 utterances met a tie in the beam search$", printed, flags=re.M)
