"""The criterion's MODULE-PREDICTOR kernel entries (cpc_infonce_forward_pred / cpc_infonce_backward_pred: K separate prediction
tensors [b, W, Henc] -- rnnMode='transformer', --multihead_rnn, 'LSTM' / 'RNN', and linear predictors under dropout) against
the fp64 oracle at the widths training runs at.  Three layers:

  1. the kernels alone on synthetic prediction tensors (cpc2_amd.criterion._InfoNCEPredFn), every selection predicate of
     nce_launch_fwd / nce_launch_bwd (csrc/infonce.hip) taken both ways at Henc 256 and 512;
  2. the same at the full batch (b = 64: the shapes of bench.py's transformer_pred / recipe configurations) against the sparse
     oracle, and against the linear family fed with the same predictions;
  3. the predictor modules through CPCUnsupersivedCriterion, the dropout route, and two steps of the documented recipe.

Which kernel a shape selects cannot be read back from the library (the profiler's slots time the forward and the backward as
one class each, whichever kernel ran), so `selection()` below restates the two predicates, every case names the pair it
expects in its id, and the test asserts that the restatement agrees: a case that drifts to another kernel fails."""
import numpy as np
import pytest
import torch

import cpc2_amd
from cpc2_amd import _lib
from cpc2_amd.criterion import _InfoNCEPredFn
from cpc2_amd.train import buildOptimizer, cpcStep
from oracle import cpc_oracle as O
from oracle import synth
from oracle.settle import settle_relu_decisions as _settle_relu_decisions
from oracle.mt19937 import MT19937, negative_indices

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_WORST = {}         # quantity -> (worst relative error seen, where)


def rel_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def assert_close(got, ref, tol, what="", rtol=None, kind=None):
    """(tests/test_recurrent_state_gpu.py) max-norm check |got - ref|_inf <= tol * |ref|_inf AND, element by element,
    |got - ref| <= atol + rtol * |ref| with atol = tol * |ref|_inf and rtol = 64 * tol by default.  `kind`: the quantity the
    error is booked under in the module's report of worst errors."""
    e = rel_err(got, ref)
    if kind is not None and e > _WORST.get(kind, (-1.0, ""))[0]:
        _WORST[kind] = (e, what)
    assert e <= tol, f"{what}: rel err {e:.3e} > {tol:.1e}"
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    atol = tol * float(r.abs().max()) + 1e-30
    rt = 64 * tol if rtol is None else rtol
    bad = (g - r).abs() > atol + rt * r.abs()
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements outside atol {atol:.2e} + {rt:.1e} |ref|"


@pytest.fixture(scope="module", autouse=True)
def _report_worst_errors():
    yield
    print("\nworst relative errors of tests/test_criterion_pred_gpu.py (run with -s):")
    for kind in sorted(_WORST):
        print(f"  {kind:<28s} {_WORST[kind][0]:.3e}   ({_WORST[kind][1]})")


# ----------------------------------------------------------------------------- which kernels a shape selects
NCE_SROW = 68           # csrc/infonce.hip: staging tile row of infonce_bwd_fused_kernel


def selection(henc, k, nn):
    """(forward, backward) kernels of nce_launch_fwd / nce_launch_bwd for a shape, restated from csrc/infonce.hip:
    forward  'dma'   infonce_fwd_dma_kernel: Henc 256 / 512, Nneg % 8 == 0, Nneg <= 256;   else 'wave' (infonce_fwd_kernel)
    backward 'fused' infonce_bwd_fused_kernel<H, ceil(K / 4)>: Henc 256 / 512, lw <= 320, Nneg % 16 == 0 and
             K (Nneg + 1) <= (Henc / 128) 16 NCE_SROW;   else 'split' (infonce_bwd_kernel + infonce_dz_store_kernel)."""
    lw = -(-(16 + nn) // 32) * 32 + 4
    wide = henc in (256, 512)
    fwd = "dma" if wide and nn % 8 == 0 and nn <= 256 else "wave"
    bwd = "fused" if wide and lw <= 320 and nn % 16 == 0 and k * (nn + 1) <= (henc // 128) * 16 * NCE_SROW else "split"
    return fwd, bwd


def _time_major(ext, b, w_len, nn):
    """negative_indices' [b, n_neg, W] order as the kernels' int32 [b, W, n_neg]."""
    return torch.as_tensor(np.asarray(ext).reshape(b, nn, w_len).transpose(0, 2, 1).copy(), dtype=torch.int32)


def _poison_free_blocks(*like):
    """Leave NaNs in the blocks the caching allocator hands out next: the backward's outputs are torch.empty buffers, and a
    kernel whose grid stops short would otherwise leave whatever an earlier (possibly identical) case had put there."""
    junk = [torch.full_like(t, float("nan")) for t in like]
    torch.cuda.synchronize()
    del junk


def _floor_quality(b, seed):
    """A signal-quality tensor [b, 9] whose last window gets the floor weight 1e-5 (criterion.py:230: 0.00001 + sigmoid)."""
    q = torch.rand(b, 9, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    q[b - 1] = -1000.0
    return q


def _run_kernels(b, t_len, henc, k, nn, seed, weights=None):
    """One call of the _pred kernels on synthetic predictions: (losses [K], acc [K], dz, [dP_k]) with the gradient of
    sum_k g_k loss_k, g = linspace(0.5, 1.5, K), plus the inputs on the host."""
    w_len = t_len - k
    z = synth.features((b, t_len, henc), seed, relu=True)
    preds = [synth.features((b, w_len, henc), seed + 1 + i, scale=2.0) for i in range(k)]
    _, _, ext = negative_indices(MT19937(seed), b, t_len, w_len, nn)
    g = torch.linspace(0.5, 1.5, k, dtype=torch.float64)
    zd = z.to(DEV).requires_grad_(True)
    pd = [p.to(DEV).requires_grad_(True) for p in preds]
    wd = None if weights is None else weights.float().to(DEV)
    losses, acc = _InfoNCEPredFn.apply(zd, _time_major(ext, b, w_len, nn).to(DEV), wd, nn, *pd)
    _poison_free_blocks(zd, *pd)
    (losses * g.float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    _lib.check(_lib.load().cpc_async_error_check(_lib.stream_ptr(zd.device)), "async errors")
    return (losses.detach(), acc.detach(), zd.grad, [p.grad for p in pd]), (z, preds, ext, g)


def _check_kernels_vs_dense_oracle(b, t_len, henc, k, nn, seed, weights=None):
    (losses, acc, dz, dps), (z, preds, ext, g) = _run_kernels(b, t_len, henc, k, nn, seed, weights)
    z64 = z.double().requires_grad_(True)
    p64 = [p.double().requires_grad_(True) for p in preds]
    dummy_c = torch.zeros(b, t_len, 1, dtype=torch.float64)
    ref_losses, ref_acc = O.criterion_forward(dummy_c, z64, [(lambda c, p=p: p) for p in p64], ext, nn, weights=weights)
    (ref_losses.view(-1) * g).sum().backward()
    tag = f"h{henc} K{k} n{nn} b{b} T{t_len}"
    assert_close(losses.view(1, -1), ref_losses, 1e-5, f"losses {tag}", kind="1 kernels: losses")
    assert torch.allclose(acc.cpu().double().view(1, -1), ref_acc, atol=2.5 / (b * (t_len - k)))     # a float tie may flip an argmax
    assert_close(dz, z64.grad, 1e-4, f"dz {tag}", kind="1 kernels: dz")
    for i in range(k):
        assert dps[i] is not None and dps[i].shape == preds[i].shape
        assert_close(dps[i], p64[i].grad, 1e-4, f"dP{i} {tag}", kind="1 kernels: dP")


# ----------------------------------------------------------------------------- 1. the kernels alone
def _case(henc, k, nn, b, t_len, fwd, bwd):
    return pytest.param(henc, k, nn, b, t_len, fwd, bwd, id=f"h{henc}-K{k}-n{nn}-b{b}-T{t_len}-{fwd}-{bwd}")


_WIDE = []
for _h in (256, 512):
    # K in every NKK = ceil(K / 4) class of the fused backward and of both parities (odd K: the `2 i + 1 < K ? .. : 0` row of the
    # unpacked request), 128 negatives: LDS-DMA forward and fused backward for every K <= 16 (16 * 129 = 2064 <= 2176)
    _WIDE += [_case(_h, _k, 128, (1, 3, 2, 5)[_i % 4], 40, "dma", "fused") for _i, _k in enumerate((1, 2, 3, 4, 5, 8, 9, 12, 13, 16))]
    # 8 / 24 negatives: LDS-DMA forward (a partial candidate tile), Nneg % 16 != 0 -> infonce_bwd_kernel + infonce_dz_store_kernel
    _WIDE += [_case(_h, 3, 8, 2, 40, "dma", "split"), _case(_h, 12, 24, 3, 40, "dma", "split"), _case(_h, 13, 24, 1, 40, "dma", "split")]
    # 17 / 129 negatives: neither fast kernel
    _WIDE += [_case(_h, 2, 17, 3, 40, "wave", "split"), _case(_h, 12, 129, 2, 40, "wave", "split"), _case(_h, 9, 129, 1, 40, "wave", "split")]
    # 288 negatives: % 16 == 0 but lw = cdiv(16 + 288, 32) * 32 + 4 = 324 > 320 -> split backward; no LDS-DMA forward (> 256)
    _WIDE += [_case(_h, 4, 288, 2, 40, "wave", "split")]
    # the windows: W = 116 (T 128, K 12), W = 1 (T = K + 1), one window, a ragged count of windows
    _WIDE += [_case(_h, 12, 128, 3, 128, "dma", "fused"), _case(_h, 12, 128, 3, 13, "dma", "fused"), _case(_h, 5, 24, 2, 6, "dma", "split"),
              _case(_h, 16, 17, 5, 17, "wave", "split")]
_WIDE += [
    # 256 negatives, lw = 292: K (Nneg + 1) against the staging tiles (2176 floats at Henc 256, 4352 at 512)
    _case(256, 8, 256, 2, 40, "dma", "fused"),          # 8 * 257 = 2056 <= 2176
    _case(256, 9, 256, 2, 40, "dma", "split"),          # 9 * 257 = 2313 >  2176
    _case(256, 16, 256, 3, 40, "dma", "split"),         # 4112 > 2176 ...
    _case(512, 16, 256, 3, 40, "dma", "fused"),         # ... but <= 4352 at Henc 512
    _case(512, 12, 256, 2, 128, "dma", "fused"),        # CPC-large's criterion shape with module predictors, W = 116
    # 272 negatives: above the LDS-DMA forward's 256 (Nneg % 8 == 0 all the same); % 16 == 0 and lw = 292 <= 320, so the staging
    # tiles alone decide the backward (nce_layout: lw = cdiv(16 + Nneg, 32) * 32 + 4)
    _case(256, 4, 272, 2, 40, "wave", "fused"),         # 4 * 273 = 1092 <= 2176
    _case(256, 8, 272, 2, 40, "wave", "split"),         # 8 * 273 = 2184 >  2176
    _case(512, 13, 272, 1, 40, "wave", "fused"),        # 13 * 273 = 3549 <= 4352
    _case(512, 16, 272, 2, 40, "wave", "split"),        # 16 * 273 = 4368 >  4352
]


@pytest.mark.parametrize("henc,k,nn,b,t_len,fwd,bwd", _WIDE)
def test_pred_kernels_at_training_widths_vs_oracle_fp64(henc, k, nn, b, t_len, fwd, bwd):
    """cpc_infonce_forward_pred / _backward_pred on K independent prediction tensors against the dense fp64 oracle: losses,
    accuracy, dz and each of the K dP, under a non-uniform gradient of the losses.  The id names the kernels the shape selects
    (selection(): forward dma / wave, backward fused / split); the unpacked request of the LDS-DMA forward (p_packed = 0),
    the p_rows = W grids and the dPk[k] stores of both backward kernels are reached by this entry only."""
    assert selection(henc, k, nn) == (fwd, bwd)
    _check_kernels_vs_dense_oracle(b, t_len, henc, k, nn, seed=1000 + 16 * henc // 256 + k + nn)


@pytest.mark.parametrize("henc,k,nn,b,t_len", [(32, 4, 8, 3, 32), (32, 16, 17, 1, 40), (64, 5, 16, 2, 40), (64, 12, 129, 3, 20),
                                               (128, 7, 24, 2, 33), (128, 13, 128, 5, 14)])
def test_pred_kernels_at_narrow_widths_vs_oracle_fp64(henc, k, nn, b, t_len):
    """Henc 32 / 64 / 128: the wave-per-(b, t) forward and the split backward in the _pred form (selection() = wave, split)."""
    assert selection(henc, k, nn) == ("wave", "split")
    _check_kernels_vs_dense_oracle(b, t_len, henc, k, nn, seed=2000 + henc + k)


@pytest.mark.parametrize("henc,k,nn,b,t_len,fwd,bwd", [_case(256, 12, 128, 3, 40, "dma", "fused"), _case(512, 9, 256, 2, 40, "dma", "fused"),
                                                       _case(512, 12, 24, 3, 40, "dma", "split"), _case(256, 5, 17, 4, 40, "wave", "split"),
                                                       _case(256, 12, 128, 3, 128, "dma", "fused"), _case(64, 4, 16, 3, 32, "wave", "split")])
def test_pred_kernels_with_quality_weights_vs_oracle_fp64(henc, k, nn, b, t_len, fwd, bwd):
    """The `weights` pointer (signal quality: one weight per window, repeated over its W frames) with module predictions, on
    the LDS-DMA + fused pair and on the split pair; the last window's weight is the floor 1e-5 (criterion.py:230)."""
    assert selection(henc, k, nn) == (fwd, bwd)
    weights = O.quality_weights(_floor_quality(b, 5), 2.0, 0.1, t_len - k)
    assert float(weights.min()) == 1e-5 and float(weights.max()) > 0.5
    _check_kernels_vs_dense_oracle(b, t_len, henc, k, nn, seed=3000 + henc + k, weights=weights)


def test_pred_function_takes_the_unbound_views_of_one_tensor():
    """prediction[:, :, k] of the multi-head predictor's [b, W, K, H] output is a strided view (criterion.py:85): the function
    has to copy it (the kernels address [b][W][H] densely) and hand the gradient back in the view's shape."""
    b, t_len, henc, k, nn = 2, 40, 256, 12, 128
    w_len = t_len - k
    z = synth.features((b, t_len, henc), 71, relu=True).to(DEV)
    stacked = synth.features((b, w_len, k, henc), 72, scale=2.0).to(DEV)
    _, _, ext = negative_indices(MT19937(73), b, t_len, w_len, nn)
    ext = _time_major(ext, b, w_len, nn).to(DEV)
    g = torch.linspace(0.5, 1.5, k, device=DEV)
    outs = []
    for contiguous in (False, True):
        zd, sd = z.clone().requires_grad_(True), stacked.clone().requires_grad_(True)
        views = list(torch.unbind(sd, dim=2))
        assert not views[0].is_contiguous()
        losses, acc = _InfoNCEPredFn.apply(zd, ext, None, nn, *([v.contiguous() for v in views] if contiguous else views))
        (losses * g).sum().backward()
        outs.append((losses.detach(), acc.detach(), zd.grad, sd.grad))
    for got, want in zip(*outs):
        assert torch.equal(got, want)


def test_pred_function_refuses_what_the_kernels_cannot_address():
    """Predictions of another shape or type, and a `weights` vector on the host or of another length, are errors -- not reads
    of whatever lies behind the pointer."""
    b, t_len, henc, k, nn = 2, 20, 64, 4, 8
    w_len = t_len - k
    z = synth.features((b, t_len, henc), 1, relu=True).to(DEV)
    preds = [synth.features((b, w_len, henc), 2 + i).to(DEV) for i in range(k)]
    _, _, ext = negative_indices(MT19937(3), b, t_len, w_len, nn)
    ext = _time_major(ext, b, w_len, nn).to(DEV)
    with pytest.raises(ValueError):
        _InfoNCEPredFn.apply(z, ext, None, nn, *(preds[:-1] + [preds[-1][:, :-1]]))
    with pytest.raises(TypeError):
        _InfoNCEPredFn.apply(z, ext, None, nn, *(preds[:-1] + [preds[-1].double()]))
    with pytest.raises(RuntimeError):
        _InfoNCEPredFn.apply(z, ext, None, nn, *(preds[:-1] + [preds[-1].cpu()]))
    with pytest.raises(RuntimeError):
        _InfoNCEPredFn.apply(z, ext, torch.ones(b * w_len), nn, *preds)
    with pytest.raises(ValueError):
        _InfoNCEPredFn.apply(z, ext, torch.ones(b * w_len - 1, device=DEV), nn, *preds)
    losses, _ = _InfoNCEPredFn.apply(z, ext, torch.ones(b * w_len, device=DEV), nn, *preds)
    assert torch.equal(losses, _InfoNCEPredFn.apply(z, ext, None, nn, *preds)[0])


# ----------------------------------------------------------------------------- 2. the full batch
_FULL = {}


def _full_batch_inputs(h, nn):
    b, t_len, k = 64, 128, 12
    if (h, nn) not in _FULL:
        cp = synth.predictor_params(k, h, h, seed=160, scale=2.0)              # trained-scale predictors (tests/test_gpu_parity.py)
        c = synth.features((b, t_len, h), 161)
        z = synth.features((b, t_len, h), 162, relu=True)
        _, _, ext = negative_indices(MT19937(4321), b, t_len, t_len - k, nn)
        _FULL[(h, nn)] = (cp, c, z, ext)
    return _FULL[(h, nn)]


@pytest.mark.parametrize("h,nn", [(256, 128), (512, 256)])
def test_pred_kernels_at_full_batch_vs_sparse_oracle(h, nn):
    """b = 64, T = 128, K = 12: the shapes of bench.py's transformer_pred / recipe configurations (Henc 256, 128 negatives) and of
    CPC-large with module predictors (512, 256) -- 7 424 (b, t) items through the persistent LDS-DMA forward (more items than
    workgroups: the next item's unpacked prediction request is in flight while this one multiplies) and a fused-backward grid
    of b * W workgroups -- against the sparse fp64 oracle fed with the same K prediction tensors (tests/test_criterion_pred_cpu.py
    holds that form to the dense oracle): losses, accuracy, every element of dz and of the K dP."""
    b, t_len, k = 64, 128, 12
    assert selection(h, k, nn) == ("dma", "fused")
    (losses, acc, dz, dps), (z, preds, ext, g) = _run_kernels(b, t_len, h, k, nn, seed=4000 + h)
    ref = O.criterion_forward_sparse(None, z.double(), [p.double() for p in preds], ext, nn, dlosses=g)
    assert_close(losses.view(1, -1), ref["losses"], 1e-5, f"losses h{h}", kind="2 full batch: losses")
    assert torch.allclose(acc.cpu().double().view(1, -1), ref["acc"], atol=2.5 / (b * (t_len - k)))
    assert_close(dz, ref["dz"], 1e-4, f"dz h{h}, all elements", kind="2 full batch: dz")
    for i in range(k):
        assert_close(dps[i], ref["dP"][i], 1e-4, f"dP{i} h{h}, all elements", kind="2 full batch: dP")


def test_pred_and_linear_families_agree_at_full_batch():
    """The same criterion through both kernel entry families at b = 64, Henc 256, 128 negatives: the linear family computes
    P_k = c W_k^T itself (cpc_infonce_forward / _backward), the _pred family is handed P_k = (c64 W_k64^T) rounded to fp32.
    Losses and dz agree to fp32 rounding (the bounds test_criterion_at_full_batch_* hold the linear family to its oracle at)."""
    lib = _lib.load()
    h, nn, b, t_len, k = 256, 128, 64, 128, 12
    w_len = t_len - k
    cp, c, z, ext = _full_batch_inputs(h, nn)
    wk = [cp[f"wPrediction.predictors.{i}.weight"] for i in range(k)]
    preds = [(c[:, :w_len].double() @ w.double().t()).float() for w in wk]
    ext_tm = _time_major(ext, b, w_len, nn).to(DEV)
    zd = z.to(DEV).requires_grad_(True)
    losses, acc = _InfoNCEPredFn.apply(zd, ext_tm, None, nn, *[p.to(DEV) for p in preds])
    losses.sum().backward()
    # the linear family, by its C entries (T context frames, the immediate backward)
    cd, wpred, z2 = c.to(DEV), torch.stack(wk).to(DEV), z.to(DEV)
    st = _lib.stream_ptr(cd.device)
    saved = torch.empty(lib.cpc_infonce_saved_bytes(b, t_len, k, h, h, nn), dtype=torch.uint8, device=DEV)
    scr = torch.empty(lib.cpc_infonce_scratch_bytes(b, t_len, k, h, h, nn), dtype=torch.uint8, device=DEV)
    lin_losses, lin_acc = torch.empty(k, device=DEV), torch.empty(k, device=DEV)
    _lib.check(lib.cpc_infonce_forward(_lib.ptr(cd), _lib.ptr(z2), _lib.ptr(wpred), _lib.ptr(ext_tm), None, _lib.ptr(lin_losses),
                                       _lib.ptr(lin_acc), _lib.ptr(saved), _lib.ptr(scr), b, t_len, t_len, k, h, h, nn, st), "fwd")
    dc, dz, dw = torch.empty_like(cd), torch.full_like(z2, float("nan")), torch.empty_like(wpred)
    ones = torch.ones(k, device=DEV)
    _lib.check(lib.cpc_infonce_backward(_lib.ptr(cd), _lib.ptr(z2), _lib.ptr(wpred), _lib.ptr(ext_tm), None, _lib.ptr(ones), _lib.ptr(saved),
                                        _lib.ptr(scr), _lib.ptr(dc), _lib.ptr(dz), _lib.ptr(dw), b, t_len, t_len, k, h, h, nn, 0, st), "bwd")
    torch.cuda.synchronize()
    _lib.check(lib.cpc_async_error_check(st), "async errors")
    assert_close(losses, lin_losses, 1e-5, "losses, _pred family vs linear family", kind="2 families: losses")
    assert torch.allclose(acc.cpu(), lin_acc.cpu(), atol=2.5 / (b * w_len))
    assert_close(zd.grad, dz, 1e-4, "dz, _pred family vs linear family", kind="2 families: dz")


# ----------------------------------------------------------------------------- 3. the predictor modules
def _multihead_once(p, k, prefix="wPrediction.predictor."):
    """O.multihead_predictors with the head evaluated once per call of the criterion (its K closures share the output)."""
    cache = {}

    def pred(c, i):
        if cache.get("c") is not c:
            cache["c"], cache["out"] = c, O.transformer_layer_forward(c, p, f"{prefix}0.", n_classifiers=k)
        return cache["out"][:, :, i]
    return [(lambda c, i=i: pred(c, i)) for i in range(k)]


def _module_criterion(kind, h, k, nn, t_len, c_w=None, **kw):
    """(criterion on the device in eval mode, its parameters by name as fp32 host tensors, p64 -> the oracle's predictors).
    c_w [b, W, h]: what the predictors will be applied to (the transformers' ReLU decisions are settled on it)."""
    if kind == "transformer":
        crit = cpc2_amd.CPCUnsupersivedCriterion(k, h, h, nn, rnnMode="transformer", sizeInputSeq=t_len, **kw)
        p = {}
        for i in range(k):
            p.update(synth.transformer_params(h, h, t_len - k, seed=80 + i, prefix=f"wPrediction.predictors.{i}.0."))
        oracle = lambda p64: O.transformer_predictors(p64, k)                                            # noqa: E731
    elif kind == "multihead":
        crit = cpc2_amd.CPCUnsupersivedCriterion(k, h, h, nn, rnnMode="transformer", sizeInputSeq=t_len, multihead_rnn=True, **kw)
        p = synth.transformer_params(h, h, t_len - k, seed=95, prefix="wPrediction.predictor.0.", n_classifiers=k)
        oracle = lambda p64: _multihead_once(p64, k)                                                     # noqa: E731
    else:
        crit = cpc2_amd.CPCUnsupersivedCriterion(k, h, h, nn, rnnMode=kind, sizeInputSeq=t_len, **kw)
        p = {}
        for i in range(k):
            p.update(synth.gru_params(h, h, 1, seed=110 + i, prefix=f"wPrediction.predictors.{i}.", gates=4 if kind == "LSTM" else 1))
        oracle = lambda p64: O.recurrent_predictors(p64, k, kind)                                        # noqa: E731
    if c_w is not None and kind == "transformer":
        for i in range(k):
            _settle_relu_decisions(p, f"wPrediction.predictors.{i}.0.", c_w)
    if c_w is not None and kind == "multihead":
        _settle_relu_decisions(p, "wPrediction.predictor.0.", c_w, n_classifiers=k)
    sd = crit.state_dict()
    assert set(p) <= set(sd) and {n for n, _ in crit.named_parameters()} == set(p)
    sd.update(p)
    crit.load_state_dict(sd)
    return crit.to(DEV).eval(), p, oracle


def _check_module_criterion(kind, h, nn, b, seed, quality=False, **kw):
    t_len, k = 128, 12
    w_len = t_len - k
    ckw = dict(kw)
    if quality:
        ckw.update(growth_rate=2.0, inflection_point_x=0.1)
    c = synth.features((b, t_len, h), seed + 1)
    z = synth.features((b, t_len, h), seed + 2, relu=True)
    c_w = (torch.flip(c, [1]) if kw.get("mode") == "reverse" else c)[:, :w_len]
    crit, p, oracle = _module_criterion(kind, h, k, nn, t_len, c_w=c_w, **ckw)
    q = _floor_quality(b, seed + 3) if quality else None
    cd, zd = c.to(DEV).requires_grad_(True), z.to(DEV).requires_grad_(True)
    crit.seed(seed)
    losses, acc = crit(cd, zd, None, None if q is None else q.float().to(DEV))
    losses.sum().backward()
    p64 = {n: v.double().requires_grad_(True) for n, v in p.items()}
    c64, z64 = c.double().requires_grad_(True), z.double().requires_grad_(True)
    _, _, ext = negative_indices(MT19937(seed), b, t_len, w_len, nn)
    okw = {key: kw[key] for key in ("mode", "n_skipped") if key in kw}
    if quality:
        okw["weights"] = O.quality_weights(q, 2.0, 0.1, w_len)
    ref_losses, ref_acc = O.criterion_forward(c64, z64, oracle(p64), ext, nn, **okw)
    ref_losses.sum().backward()
    tag = f"{kind} h{h}"
    assert losses.shape == ref_losses.shape
    assert_close(losses, ref_losses, 1e-5, f"losses {tag}", kind="3 modules: losses")
    assert torch.allclose(acc.cpu().double(), ref_acc, atol=2.5 / (b * w_len))
    assert_close(cd.grad, c64.grad, 2e-4, f"dc {tag}", kind="3 modules: dc")
    assert_close(zd.grad, z64.grad, 1e-4, f"dz {tag}", kind="3 modules: dz")
    for name, prm in crit.named_parameters():
        ref = p64[name].grad
        if ref is None or float(ref.abs().max()) == 0.0:
            assert prm.grad is None or float(prm.grad.abs().max()) == 0.0, name
        else:
            assert_close(prm.grad, ref, 5e-4, f"grad {name} {tag}", kind="3 modules: parameter gradients")


@pytest.mark.parametrize("kind", ["transformer", "multihead", "LSTM", "RNN"])
@pytest.mark.parametrize("h,nn,b", [(256, 128, 3), (512, 256, 2)])
def test_criterion_with_predictor_modules_at_training_widths_vs_oracle_fp64(kind, h, nn, b):
    """CPCUnsupersivedCriterion(...)(c, z, None) in eval mode with each family of predictor modules at Har = Henc = 256 (T 128,
    K 12, 128 negatives, b = 3) and 512 (256 negatives, b = 2) against O.criterion_forward with O.transformer_predictors /
    O.multihead_predictors (the head evaluated once) / O.recurrent_predictors: losses, accuracy, dc, dz, every parameter
    gradient.  The RNN predictors recur along the BATCH axis (nn.RNN without batch_first: oracle.recurrent_predictors), which
    b = 3 keeps visible.  The transformers' ReLU decisions are unambiguous in fp32 (_settle_relu_decisions)."""
    assert selection(h, 12, nn) == ("dma", "fused")
    _check_module_criterion(kind, h, nn, b, seed=500 + h // 256)


@pytest.mark.parametrize("name,kind,kw", [("reverse", "transformer", dict(mode="reverse")), ("skip", "multihead", dict(n_skipped=2)),
                                          ("quality", "LSTM", dict(quality=True))])
def test_criterion_with_predictor_modules_variants_vs_oracle_fp64(name, kind, kw):
    """mode='reverse' (the flip sits in front of the predictor modules), n_skipped = 2 (the kernels still run all K steps; the
    skipped steps' loss gradient is absent) and the signal-quality weights (one window at the floor) with module predictors, at
    Henc 256 / 128 negatives / b = 3."""
    _check_module_criterion(kind, 256, 128, 3, seed=600, **kw)


class _FixedMask(torch.nn.Module):
    """Stands in for nn.Dropout(0.5): the k-th call multiplies by the k-th of K fixed 0 / 2 masks."""

    def __init__(self, masks):
        super().__init__()
        self.masks, self.calls = masks, 0

    def forward(self, x):
        m = self.masks[self.calls % len(self.masks)]
        self.calls += 1
        return x * m


def test_linear_predictors_under_dropout_vs_oracle_fp64():
    """dropout=True in training mode (criterion.py:113, 168-169): the linear predictions come out of cpc_gemm_nt (_LinearFn),
    are masked and go to the _pred kernels.  With the module's dropout swapped for fixed, seeded 0 / 2 masks the route is exact:
    dense fp64 oracle with predictors c -> (c W_k^T) mask_k, at Henc 256 / 128 negatives; dc and every dW_k included."""
    h, nn, b, t_len, k = 256, 128, 3, 128, 12
    w_len = t_len - k
    crit = cpc2_amd.CPCUnsupersivedCriterion(k, h, h, nn, rnnMode="linear", dropout=True, sizeInputSeq=t_len)
    cp = synth.predictor_params(k, h, h, seed=700, scale=2.0)
    crit.load_state_dict(cp)
    crit = crit.to(DEV).train()
    gen = torch.Generator().manual_seed(701)
    masks = [(torch.rand(b, w_len, h, generator=gen) < 0.5).float() * 2.0 for _ in range(k)]
    crit.wPrediction.dropout = _FixedMask([m.to(DEV) for m in masks])
    c = synth.features((b, t_len, h), 702)
    z = synth.features((b, t_len, h), 703, relu=True)
    cd, zd = c.to(DEV).requires_grad_(True), z.to(DEV).requires_grad_(True)
    crit.seed(704)
    losses, acc = crit(cd, zd, None)
    assert crit.wPrediction.dropout.calls == k
    losses.sum().backward()
    p64 = {n: v.double().requires_grad_(True) for n, v in cp.items()}
    c64, z64 = c.double().requires_grad_(True), z.double().requires_grad_(True)
    _, _, ext = negative_indices(MT19937(704), b, t_len, w_len, nn)
    predictors = [(lambda cc, i=i: (cc @ p64[f"wPrediction.predictors.{i}.weight"].t()) * masks[i].double()) for i in range(k)]
    ref_losses, ref_acc = O.criterion_forward(c64, z64, predictors, ext, nn)
    ref_losses.sum().backward()
    assert_close(losses, ref_losses, 1e-5, "losses (dropout route)", kind="3 dropout route: losses")
    assert torch.allclose(acc.cpu().double(), ref_acc, atol=2.5 / (b * w_len))
    assert_close(cd.grad, c64.grad, 2e-4, "dc (dropout route)", kind="3 dropout route: dc")
    assert_close(zd.grad, z64.grad, 1e-4, "dz (dropout route)", kind="3 dropout route: dz")
    for i in range(k):
        assert_close(crit.wPrediction.predictors[i].weight.grad, p64[f"wPrediction.predictors.{i}.weight"].grad, 2e-4,
                     f"dW{i} (dropout route)", kind="3 dropout route: dW")


def test_recipe_two_train_steps_vs_oracle():
    """The documented recipe -- encoder 256, two LSTM layers, the multi-head transformer predictor (--multihead_rnn), 128
    negatives -- through cpcStep and buildOptimizer(...).step() at b = 2 (eval mode: parity is defined with dropout off).  Step 1:
    the losses and EVERY gradient against the fp64 oracle (O.train_step_loss with the multi-head predictors).  Step 2, after
    the update: the losses against the oracle's second step after its own Adam update, within the 1e-3 the full-step tests
    (tests/test_gpu_parity.py, _full_step_vs_oracle) allow a loss that has seen an Adam update, and every parameter against
    the oracle's within that test's bound; every parameter has moved."""
    hidden, b, k, nn, layers, lr = 256, 2, 12, 128, 2, 2e-4
    mp = synth.encoder_params(hidden, 21)
    mp.update(synth.lstm_params(hidden, hidden, layers, 26))
    model = cpc2_amd.CPCModel(cpc2_amd.CPCEncoder(hidden), cpc2_amd.CPCAR(hidden, hidden, False, layers, mode="LSTM"))
    model.load_state_dict(mp)
    x = synth.audio_windows(b, 20480, 24)
    with torch.no_grad():       # the context the predictor will see, by the oracle (the first b of the 2b windows, W frames)
        c_w = O.model_forward(torch.cat([x, x]).double(), {n: v.double() for n, v in mp.items()}, layers, "LSTM")[0][:b, :128 - k]
    crit, cp, oracle = _module_criterion("multihead", hidden, k, nn, 128, c_w=c_w)
    model = model.to(DEV)
    opt = buildOptimizer(model, crit, lr=lr)
    xd, label = x.to(DEV), torch.zeros(b, dtype=torch.long, device=DEV)
    crit.seed(79)
    tot, losses, _ = cpcStep(xd, xd, label, model, crit)
    tot.backward()
    names = list(mp) + list(cp)
    p64 = {n: (mp[n] if n in mp else cp[n]).double().requires_grad_(True) for n in names}
    mt = MT19937(79)
    ref_tot, ref_losses, _ = O.train_step_loss(x.double(), x.double(), {n: p64[n] for n in mp}, {n: p64[n] for n in cp}, mt, k, nn,
                                               layers, ar="LSTM", predictors=oracle(p64))
    ref_tot.backward()
    assert_close(losses, ref_losses, 1e-5, "losses, step 1", kind="3 recipe: losses of step 1")
    got = dict(list(model.named_parameters()) + list(crit.named_parameters()))
    assert set(got) == set(names)
    for name in names:
        assert_close(got[name].grad, p64[name].grad, 5e-4, f"grad {name}", kind="3 recipe: gradients of step 1")
    before = {n: got[n].detach().clone() for n in names}
    opt.step()
    opt.zero_grad()
    _, losses2, _ = cpcStep(xd, xd, label, model, crit)
    adam = O.Adam({n: p64[n].data for n in names}, lr=lr)
    adam.step({n: p64[n].grad for n in names})
    with torch.no_grad():
        _, ref_losses2, _ = O.train_step_loss(x.double(), x.double(), {n: p64[n] for n in mp}, {n: p64[n] for n in cp}, mt, k, nn,
                                              layers, ar="LSTM", predictors=oracle(p64))
    assert_close(losses2, ref_losses2, 1e-3, "losses, step 2", kind="3 recipe: losses of step 2")
    assert float(losses2.sum()) < float(losses.sum()) and float(ref_losses2.sum()) < float(ref_losses.sum())     # (same windows: it descends)
    # (Adam moves every weight by about lr whatever the size of its gradient, so an element whose gradient is rounding noise
    #  may end up two lr steps from the oracle's: _full_step_vs_oracle's bound, which catches a missing or mis-scaled update)
    for name in names:
        d = float((got[name].detach().double().cpu() - p64[name].detach()).abs().max())
        assert d <= 2.5 * lr + 2e-3 * float(p64[name].detach().abs().max()), f"{name}: {d:.2e}"
        assert float((got[name].detach() - before[name]).abs().max()) > 0.2 * lr, f"{name} was not updated"
