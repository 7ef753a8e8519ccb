"""The whole-utterance CTC head (csrc/ctc_head.hip through cpc2_amd/eval/common_voices_eval.py) across the domain its interface
accepts, against the fp64 statements of tests/ctc_head_oracle.py: transcriptions whose 2 L + 1 extended states pass the 256
threads of a workgroup up to the limits (1024 labels, 4096 frames), class counts on each side of a wave, the branches of
ctc_loss(), seqNorm and the strided classifier off the widths and kernel size of tests/test_common_voice_gpu.py, the gather's
second grid-stride trip, and CTCphone_criterion at the default width 256.  Every error is printed before it is asserted
(pytest -s gives the report); bounds are those of tests/test_common_voice_gpu.py, restated here."""
import functools
import math

import numpy as np
import pytest
import torch

import ctc_head_oracle as oracle
from cpc2_amd import _lib
from cpc2_amd.eval import common_voices_eval as cv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# alpha and beta are f64, so only the casts of the outputs and the f32 sum of the per-sequence losses round (the bound of
# tests/test_common_voice_gpu.py)
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


def _gemm_tol(k):
    return 2e-6 * max(1, k ** 0.5)          # tests/test_gpu_parity.py: test_gemm_nt / test_gemm_tn, k = the summed dimension


# ----------------------------------------------------------------------------- cpc_ctc_loss beyond 256 states
DEAD = 17          # "lanes65": a class whose logit is -inf in every frame and that no transcription holds


@functools.lru_cache(maxsize=None)
def _ctc_case(name):
    """(logits, input lengths, targets, target lengths, rows without an alignment)."""
    if name == "long":
        return oracle.ctc_long_case() + (oracle.CTC_LONG_INFEASIBLE,)
    if name in ("limit", "limit1024"):
        # 1024 labels: 2049 states, the limit of LDS, nine states per thread.  No two neighbours are equal, so 1024 frames align
        # (one alignment without a blank) and 1023 do not
        t = 1030 if name == "limit" else 1024
        rng = np.random.default_rng(1024)
        logits = (2 * rng.standard_normal((2, t, 5))).astype(np.float32)
        targets = np.tile(np.arange(1024) % 4, (2, 1)).astype(np.int64)
        return logits, np.array([t, 1023], np.int64), targets, np.array([1024, 1024], np.int64), (1,)
    if name == "frames":
        # the frame limit, with logits that a softmax without its maximum subtracted would overflow on
        rng = np.random.default_rng(4096)
        logits = (30 * rng.standard_normal((1, 4096, 6))).astype(np.float32)
        return logits, np.array([4096], np.int64), rng.integers(0, 5, (1, 8)).astype(np.int64), np.array([8], np.int64), ()
    assert name.startswith("lanes")
    # the blank (k - 1) and the log-sum-exp's lane loop on each side of a wave of 64; k = 2 is the smallest class count
    k = int(name[5:])
    rng = np.random.default_rng(k)
    logits = (2 * rng.standard_normal((4, 40, k))).astype(np.float32)
    targets = rng.integers(0, k - 1, (4, 6))
    targets[1, :3] = targets[1, 0]                      # a repeated label
    if k == 65:
        targets[targets == DEAD] = DEAD + 1
        logits[:, :, DEAD] = -np.inf
    return logits, np.array([40, 33, 1, 40], np.int64), targets.astype(np.int64), np.array([5, 4, 1, 0], np.int64), ()


@functools.lru_cache(maxsize=None)
def _ctc_ref(name, reduction):
    logits, in_len, targets, tgt_len, _ = _ctc_case(name)
    return oracle.ctc_len(logits, in_len, targets, tgt_len, reduction)


def _ctc_run(logits, in_len, targets, tgt_len, reduction, grad=True):
    lib = _lib.load()
    b, t, k = logits.shape
    lg, il, tg, tl = _dev(logits), _dev(in_len), _dev(targets), _dev(tgt_len)
    nll = torch.full((b,), 7.0, device=DEV)
    loss = torch.full((1,), 7.0, device=DEV)
    dl = torch.full_like(lg, 7.0) if grad else None
    nb = lib.cpc_ctc_loss_scratch_bytes(b, t, targets.shape[1])
    assert nb > 0
    sc = torch.empty(nb, dtype=torch.uint8, device=DEV)
    _lib.check(lib.cpc_ctc_loss(_p(lg), b, t, k, _p(il), _p(tg) if targets.shape[1] else None, targets.shape[1], _p(tl),
                                {"sum": 0, "mean": 1}[reduction], _p(nll), _p(loss), _p(dl), _p(sc), nb, _st()), "ctc_loss")
    return float(loss), nll.cpu().numpy(), None if dl is None else dl.cpu().numpy()


def _ctc_errors(tag, loss, grad, ref_loss, ref_grad, nll=None, ref_nll=None):
    """Prints and asserts loss, nll and the gradient ROW BY ROW, each row against its own largest reference element: under the
    mean reduction a row with few labels has a gradient a hundred times that of a long row, and a batch-wide norm would hide an
    error confined to the long one."""
    e_loss = abs(loss - ref_loss) / abs(ref_loss)
    rows = [float(np.abs(g - r).max() / np.abs(r).max()) if np.abs(r).max() > 0 else float(np.abs(g).max())
            for g, r in zip(grad.astype(np.float64), ref_grad)]
    text = f"{tag}: loss {e_loss:.2e}"
    if nll is not None:
        live = ref_nll > 0
        e_nll = float((np.abs(nll - ref_nll)[live] / ref_nll[live]).max())
        text += f" nll {e_nll:.2e} (nll {ref_nll[live].min():.4g} .. {ref_nll.max():.4g})"
    print(text + f" grad, worst row {max(rows):.2e}; by row " + " ".join(f"{e:.1e}" for e in rows) +
          "; largest |grad| by row " + " ".join(f"{np.abs(r).max():.1e}" for r in ref_grad))
    assert e_loss <= CTC_TOL
    if nll is not None:
        assert np.all(np.abs(nll - ref_nll) <= CTC_TOL * np.abs(ref_nll))
    for row, e in enumerate(rows):
        assert e <= CTC_TOL, row


CTC_CASES = ["long", "limit", "frames", "lanes2", "lanes63", "lanes64", "lanes65", "lanes1000"]


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("name", CTC_CASES)
def test_ctc_loss_vs_fp64_across_the_domain(name, reduction):
    logits, in_len, targets, tgt_len, infeasible = _ctc_case(name)
    ref_loss, ref_nll, ref_grad = _ctc_ref(name, reduction)
    b = logits.shape[0]
    # the oracle's side first: which rows have an alignment (a changed seed cannot empty a case)
    for row in range(b):
        assert (ref_nll[row] == 0) == (row in infeasible), row
        assert (ref_grad[row] == 0).all() == (row in infeasible), row
    assert np.isfinite(ref_grad).all() and math.isfinite(ref_loss) and ref_loss > 0
    if name == "long":
        assert (2 * tgt_len[:8] + 1 > 256).all() and ref_nll.max() > 800
    if name == "limit":
        assert 2 * targets.shape[1] + 1 == 2049 and (tgt_len == 1024).all() and ref_nll[0] > 2000
    if name == "frames":
        assert logits.shape[1] == 4096 and np.abs(logits).max() > 89 and ref_nll[0] > 1e5      # (exp(89) overflows an f32)
    if name == "lanes65":
        assert np.isneginf(logits[:, :, DEAD]).all() and not (targets == DEAD).any() and (ref_grad[:, :, DEAD] == 0).all()

    loss, nll, grad = _ctc_run(logits, in_len, targets, tgt_len, reduction)
    _ctc_errors(f"ctc {name} {reduction}", loss, grad, ref_loss, ref_grad, nll, ref_nll)
    assert not np.isnan(grad).any() and not np.isnan(nll).any()
    for row in range(b):                              # exactly 0 beyond each input length, and for the rows without an alignment
        assert (grad[row, in_len[row]:] == 0).all(), row
        if row in infeasible:
            assert nll[row] == 0 and (grad[row] == 0).all(), row
    if name == "lanes65":
        assert (grad[:, :, DEAD] == 0).all()
    # identical bits on a second launch, and without the gradient buffer
    loss2, nll2, grad2 = _ctc_run(logits, in_len, targets, tgt_len, reduction)
    assert loss2 == loss and np.array_equal(nll2, nll) and np.array_equal(grad2, grad)
    loss3, nll3, _ = _ctc_run(logits, in_len, targets, tgt_len, reduction, grad=False)
    assert loss3 == loss and np.array_equal(nll3, nll)


@pytest.mark.parametrize("name", ["long", "limit1024"])
def test_ctc_loss_with_full_lengths_equals_probe_ctc_bit_for_bit_past_256_states(name):
    """tests/test_common_voice_gpu.py's comparison with probe_ctc_kernel, where a thread owns several states (cpc_probe_ctc takes
    at most 1024 frames, so the limit of 1024 labels runs in exactly 1024 frames: one alignment per row)."""
    lib = _lib.load()
    logits, _, targets, tgt_len, _ = _ctc_case(name)
    b, t, k = logits.shape
    full = np.full(b, t, np.int64)
    loss, nll, grad = _ctc_run(logits, full, targets, tgt_len, "mean")
    lg, tg, tl = _dev(logits), _dev(targets), _dev(tgt_len)
    p_nll, p_loss, p_grad = torch.empty(b, device=DEV), torch.empty(1, device=DEV), torch.empty_like(lg)
    nb = lib.cpc_probe_ctc_scratch_bytes(b, t, targets.shape[1])
    assert nb > 0
    sc = torch.empty(nb, dtype=torch.uint8, device=DEV)
    _lib.check(lib.cpc_probe_ctc(_p(lg), b, t, k, _p(tg), targets.shape[1], _p(tl), _p(p_nll), _p(p_loss), _p(p_grad), _p(sc), nb,
                                 _st()), "probe_ctc")
    assert loss == float(p_loss) and np.array_equal(nll, p_nll.cpu().numpy()) and np.array_equal(grad, p_grad.cpu().numpy())
    ref_loss, ref_nll, ref_grad = oracle.ctc_len(logits, full, targets, tgt_len, "mean")
    assert (ref_nll > 0).all()                           # (with all of the frames every row of both cases has an alignment)
    _ctc_errors(f"ctc {name}, full lengths", loss, grad, ref_loss, ref_grad, nll, ref_nll)
    assert np.isfinite(grad).all() and (nll > 0).all()


# ----------------------------------------------------------------------------- ctc_loss() and _CTCLossFn
def _py_ctc(logits, in_len, targets, tgt_len, reduction="mean", factor=None, grad=True, tables=torch.int64):
    """(loss, dlogits) through cv.ctc_loss and autograd; `factor` scales the loss before backward."""
    lg = _dev(logits).requires_grad_(grad)
    loss = cv.ctc_loss(lg, _dev(in_len, tables), _dev(targets, tables), _dev(tgt_len, tables), reduction)
    assert tuple(loss.shape) == (1,)
    if not grad:
        assert not loss.requires_grad
        return float(loss), None
    (loss if factor is None else factor * loss).sum().backward()
    return float(loss.detach()), lg.grad.cpu().numpy()


@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_ctc_loss_wrapper_targets_wider_than_the_frames(reduction):
    rng = np.random.default_rng(12)
    logits = (2 * rng.standard_normal((3, 12, 6))).astype(np.float32)
    targets = rng.integers(0, 5, (3, 20))
    in_len, tgt_len = np.array([12, 12, 12]), np.array([5, 15, 20])
    ref_loss, ref_nll, ref_grad = oracle.ctc_len(logits, in_len, targets, tgt_len, reduction)
    assert ref_nll[0] > 0 and ref_nll[1] == 0 and ref_nll[2] == 0       # 15 and 20 labels have no alignment in 12 frames
    loss, grad = _py_ctc(logits, in_len, targets, tgt_len, reduction)
    _ctc_errors(f"ctc_loss() W=20 > T=12 {reduction}", loss, grad, ref_loss, ref_grad)
    assert (grad[1:] == 0).all()
    # a target length beyond the GIVEN width stays the kernel's NaN, and the other rows keep their bits
    bad_loss, bad_grad = _py_ctc(logits, in_len, targets, np.array([5, 15, 21]), reduction)
    assert math.isnan(bad_loss) and np.isnan(bad_grad[2]).all() and np.array_equal(bad_grad[:2], grad[:2])


def test_ctc_loss_wrapper_cuts_wide_targets_to_the_kernels_limit():
    assert cv.MAX_TARGET == 1024
    rng = np.random.default_rng(1100)
    logits = (2 * rng.standard_normal((1, 1100, 4))).astype(np.float32)
    targets = (np.arange(1030) % 3)[None]
    ref_loss, ref_nll, ref_grad = oracle.ctc_len(logits, [1100], targets, [1024], "mean")
    assert ref_nll[0] > 0
    loss, grad = _py_ctc(logits, [1100], targets, [1024])
    _ctc_errors("ctc_loss() W=1030, 1024 labels", loss, grad, ref_loss, ref_grad)
    with pytest.raises(ValueError, match=r"1025 labels.*1024"):
        _py_ctc(logits, [1100], targets, [1025])


def test_ctc_loss_wrapper_input_forms_and_upstream_gradient():
    rng = np.random.default_rng(77)
    logits = (2 * rng.standard_normal((3, 21, 7))).astype(np.float32)
    targets = rng.integers(0, 6, (3, 8))
    in_len, tgt_len = np.array([21, 13, 20]), np.array([6, 3, 8])
    ref_loss, ref_nll, ref_grad = oracle.ctc_len(logits, in_len, targets, tgt_len, "mean")
    assert (ref_nll > 0).all()
    loss, grad = _py_ctc(logits, in_len, targets, tgt_len)
    _ctc_errors("ctc_loss() forms", loss, grad, ref_loss, ref_grad)
    # int32 tables
    loss32, grad32 = _py_ctc(logits, in_len, targets, tgt_len, tables=torch.int32)
    assert loss32 == loss and np.array_equal(grad32, grad)
    # logits that are a permuted view of a [T, B, K] tensor
    base = _dev(np.ascontiguousarray(logits.transpose(1, 0, 2))).requires_grad_()
    view = base.permute(1, 0, 2)
    assert not view.is_contiguous()
    loss_v = cv.ctc_loss(view, _dev(in_len), _dev(targets), _dev(tgt_len), "mean")
    loss_v.sum().backward()
    assert float(loss_v.detach()) == loss and np.array_equal(base.grad.permute(1, 0, 2).cpu().numpy(), grad)
    # logits that need no gradient
    assert _py_ctc(logits, in_len, targets, tgt_len, grad=False)[0] == loss
    # an upstream gradient of 3: exactly three times each element (one f32 product), and the oracle's
    loss3, grad3 = _py_ctc(logits, in_len, targets, tgt_len, factor=3.0)
    assert loss3 == loss and np.array_equal(grad3, np.float32(3.0) * grad) and np.abs(grad3).max() > 0
    _ctc_errors("ctc_loss() upstream gradient 3", loss3, grad3, ref_loss, 3.0 * ref_grad)


# ----------------------------------------------------------------------------- normalisation over the first len frames
# The element-by-element first-order f32 bound of tests/test_common_voice_gpu.py (derived there): the statistics are summed in f64,
# so with u = 2^-24
#   |y err|     <= u |y|
#   |dx err[f]| <= u (2 |dx[f]| + [f < n] rstd |y[f]| / (n - 1) (|B| + sum_g |dy[g] y[g]|)),  B = sum_g dy[g] y[g]
# SLACK covers eps arriving as an f32 and the f64 sums; FLOOR an element that cancels to nothing.  (That module's 2e-6 absolute
# bound was stated for s = 40 and is not carried over: the absolute error is printed.)
U = 2.0 ** -24
SLACK = 1e-8
FLOOR = 1e-12


def _seqnorm_check(tag, x, dy, lengths, y, dx, mean=None, rstd=None):
    ref_y = oracle.seqnorm_len(x, lengths)
    ref_dx = oracle.seqnorm_len_backward(x, lengths, dy)
    s = x.shape[1]
    for i, n in enumerate(lengths):
        assert 2 <= n <= s
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
        print(f"{tag} len={n}: y {ey.max():.2e} abs, {(ey / bound_y).max():.2f} of the bound (max |y| {np.abs(ref_y[i]).max():.1e}); "
              f"dx {ex.max():.2e} abs, {(ex / bound_dx).max():.2f} of the bound (max |dx| {np.abs(ref_dx[i]).max():.1e})")
        assert (ey <= bound_y).all() and (ex <= bound_dx).all()
        if mean is not None:
            # the saved statistics against the oracle's, and with them: frames at or beyond len are normalised like the others
            assert (np.abs(mean[i] - m) <= U * np.abs(m) + FLOOR).all()
            assert (np.abs(rstd[i] - r) <= (U + SLACK) * r).all()
        assert (np.abs(y[i, n:] - ((x64 - m) * r)[n:]) <= bound_y[n:]).all()


def _seqnorm_inputs(b, s, h, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((b, s, h)) * (1 + np.arange(h) / h) + np.linspace(-2, 2, h)).astype(np.float32)
    return x, rng.standard_normal((b, s, h)).astype(np.float32)


# h neither below 64 nor a multiple of it (a workgroup owns 64 channels), fewer frames than the four waves that share them, one
# utterance, one channel, and long s
SEQNORM_SHAPES = [(1, 3, 65, [3]), (2, 2, 1, [2, 2]), (3, 5, 100, [5, 2, 3]), (2, 2000, 63, [2000, 1501]), (2, 257, 320, [257, 2])]


@pytest.mark.parametrize("b,s,h,lengths", SEQNORM_SHAPES, ids=[f"{b}x{s}x{h}" for b, s, h, _ in SEQNORM_SHAPES])
def test_seqnorm_len_vs_fp64_across_the_domain(b, s, h, lengths):
    lib = _lib.load()
    x, dy = _seqnorm_inputs(b, s, h, 1000 * s + h)
    xd, dyd, ln = _dev(x), _dev(dy), _dev(lengths, torch.int64)

    def run():
        y, dx = torch.full_like(xd, 7.0), torch.full_like(xd, 7.0)
        mean, rstd = torch.full((b, h), 7.0, device=DEV), torch.full((b, h), 7.0, device=DEV)
        _lib.check(lib.cpc_seqnorm_len_forward(_p(xd), _p(ln), b, s, h, 1e-8, _p(y), _p(mean), _p(rstd), _st()), "seqnorm_len_forward")
        _lib.check(lib.cpc_seqnorm_len_backward(_p(dyd), _p(y), _p(rstd), _p(ln), b, s, h, _p(dx), _st()), "seqnorm_len_backward")
        return y.cpu().numpy(), dx.cpu().numpy(), mean.cpu().numpy(), rstd.cpu().numpy()

    y, dx, mean, rstd = run()
    _seqnorm_check(f"seqnorm b={b} s={s} h={h}", x, dy, lengths, y, dx, mean.astype(np.float64), rstd.astype(np.float64))
    for a, again in zip((y, dx, mean, rstd), run()):       # identical bits on a second launch
        assert np.array_equal(a, again)


def test_seqnorm_len_fn_with_a_permuted_input_and_an_upstream_gradient():
    b, s, h, lengths = 2, 9, 100, [9, 4]
    x, dy = _seqnorm_inputs(b, s, h, 9100)
    base = _dev(np.ascontiguousarray(x.transpose(0, 2, 1))).requires_grad_()          # [b, h, s]
    view = base.permute(0, 2, 1)
    assert not view.is_contiguous()
    y = cv._SeqNormLenFn.apply(view, _dev(lengths, torch.int64), 1e-8)
    y.backward(_dev(dy))
    _seqnorm_check("_SeqNormLenFn h=100", x, dy, lengths, y.detach().cpu().numpy(), base.grad.permute(0, 2, 1).cpu().numpy())


# ----------------------------------------------------------------------------- the strided classifier
# (b, s, h, c, ks): P = 1 at stride 1 with one class; stride 1; a frame left over with lda = stride h = 130; P = 1 with more
# than 64 classes; frames left over at ks = 16; the default width (K = ks h = 2048 is split) with 149 rows and s % 4 = 3
CONV_SHAPES = [(2, 2, 5, 1, 2), (3, 9, 100, 7, 2), (2, 13, 65, 3, 4), (1, 16, 32, 70, 16), (2, 45, 32, 42, 16), (2, 603, 256, 42, 8)]


@pytest.mark.parametrize("b,s,h,c,ks", CONV_SHAPES, ids=["x".join(map(str, shape)) for shape in CONV_SHAPES])
def test_conv_head_vs_fp64_across_the_domain(b, s, h, c, ks):
    rng = np.random.default_rng(1000 * s + 10 * h + ks)
    x = rng.standard_normal((b, s, h)).astype(np.float32)
    w = (rng.standard_normal((c, h, ks)) / 16).astype(np.float32)
    bias = rng.standard_normal(c).astype(np.float32)
    stride = ks // 2
    p = (s - ks) // stride + 1
    dout = rng.standard_normal((b, p, c)).astype(np.float32)
    ref = oracle.conv_head(x, w, bias)
    ref_dw, ref_db, ref_dx = oracle.conv_head_backward(x, w, dout)
    assert ref.shape == (b, p, c) and (ref_dx[:, stride * (p + 1):] == 0).all() and np.abs(ref_dx[:, :stride * (p + 1)]).min() > 0

    def run():
        xd, wd, bd = (_dev(a).requires_grad_() for a in (x, w, bias))
        out = cv._ConvHeadFn.apply(xd, wd, bd)
        assert tuple(out.shape) == (b, p, c)
        out.backward(_dev(dout))
        return dict(out=out.detach().cpu().numpy(), dW=wd.grad.cpu().numpy(), db=bd.grad.cpu().numpy(), dx=xd.grad.cpu().numpy())

    got = run()
    tols = dict(out=_gemm_tol(ks * h), dW=_gemm_tol(b * p), db=_gemm_tol(b * p), dx=_gemm_tol(2 * c))
    errs = dict(out=_rel(got["out"], ref), dW=_rel(got["dW"], ref_dw), db=_rel(got["db"], ref_db), dx=_rel(got["dx"], ref_dx))
    print(f"conv head b={b} s={s} h={h} c={c} ks={ks} (P={p}): " + " ".join(f"{k} {errs[k]:.2e}/{tols[k]:.1e}" for k in errs))
    for name in errs:
        assert errs[name] <= tols[name], name
    assert (got["dx"][:, stride * (p + 1):] == 0).all()    # the frames left over belong to no output frame
    again = run()                                          # identical bits on a second run, the K split included
    for name in got:
        assert np.array_equal(got[name], again[name]), name


# ----------------------------------------------------------------------------- the utterance gather
def _gather_ref(pack, offsets, lengths, roffset, max_len):
    ref = np.zeros((len(offsets), max_len), np.float32)
    for i in range(len(offsets)):
        if offsets[i] + lengths[i] <= len(pack) and roffset[i] <= lengths[i]:
            row = pack[offsets[i] + roffset[i]:offsets[i] + lengths[i]][:max_len]
            ref[i, :len(row)] = row
    return ref


def test_gather_utterances_past_the_grid_stride_boundary():
    """gather_utt_kernel caps its grid at 1024 workgroups of 256 and strides: the second trip starts at sample 262 144."""
    edge = 1024 * 256
    rng = np.random.default_rng(2)
    pack = rng.standard_normal(700_000).astype(np.float32)
    assert (pack != 0).all()
    # item 0 is longer than max_len (cut); item 1 is shorter than the boundary (zeros on both of its sides); item 2 starts at
    # a random offset and its samples cross the boundary
    offsets = np.array([0, 320_000, 420_000], np.int64)
    lengths = np.array([320_000, 100_000, 280_000], np.int64)
    roffset = np.array([0, 0, int(rng.integers(1, 5000))], np.int64)
    max_len = 300_001
    assert max_len > edge and lengths[0] > max_len and lengths[1] < edge < lengths[2] - roffset[2] < max_len
    ref = _gather_ref(pack, offsets, lengths, roffset, max_len)
    out = cv.gather_utterances(_dev(pack), _dev(offsets), _dev(lengths), _dev(roffset), max_len).cpu().numpy()
    assert out.shape == ref.shape and np.array_equal(out, ref)
    assert (ref[0] != 0).all() and (ref[1, 100_000:] == 0).all() and (ref[2, edge:lengths[2] - roffset[2]] != 0).all()
    one = cv.gather_utterances(_dev(pack), _dev(offsets[2:]), _dev(lengths[2:]), _dev(roffset[2:]), edge + 1).cpu().numpy()
    assert one.shape == (1, edge + 1) and np.array_equal(one, _gather_ref(pack, offsets[2:], lengths[2:], roffset[2:], edge + 1))
    assert one[0, edge] != 0


# ----------------------------------------------------------------------------- CTCphone_criterion at the default width
CRIT_H, CRIT_PHONES, CRIT_KS = 256, 41, 8


@functools.lru_cache(maxsize=None)
def _criterion_case(lstm):
    rng = np.random.default_rng(320)
    c = rng.standard_normal((3, 320, CRIT_H)).astype(np.float32)
    sizes = np.array([320, 257, 131])
    label = rng.integers(0, CRIT_PHONES, (3, 70))
    label[0] = np.arange(70) % CRIT_PHONES               # 70 labels in 79 frames: no neighbours equal
    label[1, 3:6] = label[1, 3]                          # repeated labels
    label_size = np.array([70, 40, 1])
    with torch.random.fork_rng(devices=[]):              # a seeded init that leaves the session's generator as it was
        torch.manual_seed(256 + lstm)
        state = {k: v.numpy().copy() for k, v in
                 cv.CTCphone_criterion(CRIT_H, CRIT_PHONES, LSTM=lstm, sizeKernel=CRIT_KS, seqNorm=True).state_dict().items()}
    return c, sizes, label, label_size, state


@functools.lru_cache(maxsize=None)
def _criterion_ref(lstm, reduction):
    c, sizes, label, label_size, state = _criterion_case(lstm)
    return oracle.criterion(c, sizes, state, True, lstm, label, label_size, reduction)


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("lstm", [False, True])
def test_criterion_at_the_default_width_vs_fp64(lstm, reduction):
    c, sizes, label, label_size, state = _criterion_case(lstm)
    ref = _criterion_ref(lstm, reduction)
    assert ref["pred"].shape == (3, 79, CRIT_PHONES + 1) and (ref["nll"] > 0).all() and ref["loss"] > 0
    crit = cv.CTCphone_criterion(CRIT_H, CRIT_PHONES, LSTM=lstm, sizeKernel=CRIT_KS, seqNorm=True, reduction=reduction)
    crit.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    crit.to(DEV).eval()
    cd = _dev(c).requires_grad_()
    sz = _dev(sizes)
    e_pred = _rel(crit.getPrediction(cd, sz).detach().cpu(), ref["pred"])
    loss = crit(cd, sz, _dev(label), _dev(label_size))
    assert tuple(loss.shape) == (1, 1)
    loss.mean().backward()
    e_loss = abs(float(loss.detach()) - ref["loss"]) / abs(ref["loss"])
    e_dc = _rel(cd.grad.cpu(), ref["dc"])
    used = [k for k in state if lstm or not k.startswith("conv1.")]
    e_par = {k: _rel(dict(crit.named_parameters())[k].grad.cpu(), ref["grads"][k]) for k in used}
    tol = max(1e-5, _gemm_tol(CRIT_KS * CRIT_H))
    print(f"criterion h={CRIT_H} LSTM={lstm} {reduction}: pred {e_pred:.2e}/{tol:.1e} loss {e_loss:.2e}/{tol:.1e} dc {e_dc:.2e}/1.0e-04 " +
          " ".join(f"{k.split('.')[-1]} {e:.2e}" for k, e in e_par.items()))
    assert e_pred <= tol and e_loss <= tol
    assert e_dc <= 1e-4
    for k, e in e_par.items():
        assert np.abs(ref["grads"][k]).max() > 0 and e <= 1e-4, k
    if not lstm:
        assert all(p.grad is None for k, p in crit.named_parameters() if k.startswith("conv1."))
