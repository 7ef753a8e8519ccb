"""Drop-in counterpart of the reference's unsupervised CPC criterion.

Mirrors /root/reference/cpc/criterion/criterion.py: PredictionNetwork (:97-173, linear branch
:144-150), BaseCriterion (:176-183), NoneCriterion (:185-191), CPCUnsupersivedCriterion (:193-363)
-- same constructor/forward signatures, attribute names and state-dict keys
(`wPrediction.predictors.{k}.weight`).  The K candidate tensors of sampleClean (:237-286) are never
materialised: the fused HIP kernel gathers negatives on the fly from the index stream.  The supervised probe criteria of the
linear-separability evaluation (SpeakerCriterion, PhoneCriterion, CTCPhoneCriterion, criterion.py:366-495) sit at the end, on
the loss heads of csrc/probe.hip.

Negative indices are drawn on the HOST with the same MT19937 stream torch's CPU generator would
produce (the reference's CPU path); by default the criterion consumes -- and advances -- torch's
global CPU generator, so `torch.manual_seed(s)` gives bit-identical indices to the reference.
"""
import ctypes
import os

import torch
import torch.nn as nn

from . import _lib
from ._lib import check, f32c, grad_buffers, ptr, require_gpu, scratch, stream_ptr
from ._route import DeferScope, cached_grad_buffer, grad_home, grad_home_view, join_deferred, keep_deferred, mark
from .sampler import NegativeSampler  # noqa: F401  (its home is sampler.py; importers find it here as before)


# --------------------------------------------------------------------------- fused InfoNCE
def _packed_view(tensors):
    """[K, *shape] view over K equally shaped tensors that sit back to back in memory (the predictors of a
    FlatAdam-managed criterion do), else None."""
    first = tensors[0]
    step = first.numel() * first.element_size()
    need = first.storage_offset() * first.element_size() + len(tensors) * step
    if first.untyped_storage().nbytes() < need:          # adjacent by accident, not one allocation
        return None
    for i, t in enumerate(tensors):
        if not t.is_contiguous() or t.shape != first.shape or t.data_ptr() != first.data_ptr() + i * step:
            return None
    k = len(tensors)
    return torch.as_strided(first, (k,) + tuple(first.shape), (first.numel(),) + tuple(first.stride()))


def _infonce_forward(z, ext_idx, weights, n_neg, c=None, wpred=None, preds=None):
    """The one launch of the fused InfoNCE forward: z [b, t, dim_enc], ext_idx int32 [b, W, n_neg], weights [b * W] or None, and
    either c [b, t or W, dim_ar] with the packed predictor weights wpred [K, dim_enc, dim_ar] (the kernel forms the predictions)
    or the K prediction tensors preds [b, W, dim_enc]; float tensors fp32 and contiguous.  Returns (losses [K], acc [K], saved)."""
    lib = _lib.load()
    if preds is None:
        b, tc, dim_ar = c.shape
        k, dim_enc, _ = wpred.shape
        t = z.shape[1]
        # c holds the t frames of the sequence, or only the W = t - k the criterion uses (criterion.py:296: cFeature[:, :windowSize])
        if z.shape != (b, t, dim_enc) or wpred.shape[2] != dim_ar or tc not in (t, t - k):
            raise ValueError(f"shape mismatch c={tuple(c.shape)} z={tuple(z.shape)} W={tuple(wpred.shape)}")
    else:
        b, t, dim_enc = z.shape
        k, dim_ar = len(preds), dim_enc
        if any(p.shape != (b, t - k, dim_enc) for p in preds):
            raise ValueError(f"predictions must be [b, W, dim_enc] = {(b, t - k, dim_enc)}")
    if ext_idx.dtype != torch.int32 or ext_idx.numel() != b * n_neg * (t - k):
        raise ValueError("ext_idx must be int32 [b, W, n_neg]")
    if weights is not None and weights.numel() != b * (t - k):
        raise ValueError(f"weights must hold one value per (window, frame): {b * (t - k)}, got {weights.numel()}")
    nsaved = lib.cpc_infonce_saved_bytes(b, t, k, dim_ar, dim_enc, n_neg)
    # (-dim_ar: the linear entry points' own need -- without the contribution rows where dz comes from per-row context sums)
    nscratch = lib.cpc_infonce_scratch_bytes(b, t, k, -dim_ar if preds is None else dim_ar, dim_enc, n_neg)
    if nsaved == 0:
        check(-1, "infonce shape query")
    losses = torch.empty(k, dtype=torch.float32, device=z.device)
    acc = torch.empty(k, dtype=torch.float32, device=z.device)
    saved = torch.empty(nsaved, dtype=torch.uint8, device=z.device)
    sc = scratch(nscratch, z.device)
    if preds is None:
        check(lib.cpc_infonce_forward(ptr(c), ptr(z), ptr(wpred), ptr(ext_idx), ptr(weights), ptr(losses), ptr(acc),
                                      ptr(saved), ptr(sc), b, t, tc, k, dim_ar, dim_enc, n_neg, stream_ptr(z.device)), "infonce_forward")
    else:
        check(lib.cpc_infonce_forward_pred(_lib.ptr_array(preds), ptr(z), ptr(ext_idx), ptr(weights), ptr(losses), ptr(acc),
                                           ptr(saved), ptr(sc), b, t, k, dim_enc, n_neg, stream_ptr(z.device)),
              "infonce_forward_pred")
    return losses, acc, saved


class _InfoNCEFn(torch.autograd.Function):
    """inputs: c, z, ext_idx, weights, n_neg, defer, then the K predictor weights [dim_enc, dim_ar].  defer: None, or
    (start, n): the criterion's targets are windows start .. start + n of z and the backward is the deferred one."""

    @staticmethod
    def forward(ctx, c, z, ext_idx, weights, n_neg, defer, *wk):
        require_gpu(c, z, ext_idx, weights, *wk)
        ctx.c_home = grad_home(c)              # (first_windows: dc goes where the slice's backward looks for it, the rest stays zero)
        c = f32c(c)
        ctx.z_full_shape = None
        ctx.z_home = grad_home(z)              # (split_windows: dz is written where the split's backward looks for it)
        if defer is not None:
            ctx.z_full_shape, ctx.z_start = tuple(z.shape), defer[0]
            z = z[defer[0]:defer[0] + defer[1]]
        z = f32c(z)
        wpred = _packed_view([w.detach() for w in wk])
        if wpred is None:
            wpred = torch.stack([f32c(w.detach()) for w in wk], dim=0)
        w = f32c(weights) if weights is not None else None
        losses, acc, saved = _infonce_forward(z, ext_idx, w, n_neg, c=c, wpred=wpred)
        ctx.save_for_backward(c, z, wpred, ext_idx, w, saved)
        ctx.param_refs = wk
        ctx.dims = (c.shape[0], z.shape[1], wpred.shape[0], c.shape[2], z.shape[2], n_neg)
        ctx.mark_non_differentiable(acc)
        ctx.set_materialize_grads(False)       # (no zeros tensor -- a launch -- for the gradient of `acc`, which nobody has)
        return losses, acc

    @staticmethod
    def backward(ctx, dlosses, _dacc):
        lib = _lib.load()
        c, z, wpred, ext_idx, w, saved = ctx.saved_tensors
        b, t, k, dim_ar, dim_enc, n_neg = ctx.dims
        if dlosses is None:                    # (materialize_grads is off: a loss nobody differentiated)
            dlosses = torch.zeros(k, dtype=torch.float32, device=c.device)
        dlosses = f32c(dlosses)
        dc = grad_home_view(ctx.c_home, c)
        defer = ctx.z_full_shape is not None
        if defer and ctx.z_full_shape != tuple(z.shape):
            # (windows outside start .. start + n get no gradient from the criterion: zero once, see cached_grad_buffer)
            dz_out = cached_grad_buffer(ctx.z_full_shape, z.device, ("targets", ctx.z_start, z.shape[0]))
            dz = dz_out[ctx.z_start:ctx.z_start + z.shape[0]]
        else:
            dz_out = dz = grad_home_view(ctx.z_home, z)
        gw = grad_buffers(ctx.param_refs)
        dw = _packed_view(gw)                 # contiguous in the flat gradient buffer -> written in place
        direct = dw is not None
        if not direct:
            dw = torch.empty_like(wpred)
        nscratch = lib.cpc_infonce_scratch_bytes(b, t, k, -dim_ar, dim_enc, n_neg)
        # (the weight gradients may only be late when nothing reads them before the end of the backward pass: written in place
        #  into the flat gradient buffer.  A private buffer is added to .grad by autograd as soon as this function returns.)
        defer = defer and direct
        if defer:
            join_deferred(c.device)            # (one pending backward per device)
        sc = scratch(nscratch, c.device, tag="infonce_deferred") if defer else scratch(nscratch, c.device)
        check(lib.cpc_infonce_backward(ptr(c), ptr(z), ptr(wpred), ptr(ext_idx), ptr(w), ptr(dlosses), ptr(saved), ptr(sc), ptr(dc),
                                       ptr(dz), ptr(dw), b, t, c.shape[1], k, dim_ar, dim_enc, n_neg, int(defer), stream_ptr(c.device)),
              "infonce_backward")
        if defer:
            keep_deferred(c.device, (c, z, wpred, ext_idx, w, dlosses, saved, sc, dz_out, dw))
        if not direct:
            gw = list(dw.unbind(0))
        return (dc, dz_out, None, None, None, None) + tuple(gw)


class _InfoNCEPredFn(torch.autograd.Function):
    """Same criterion, predictions supplied by predictor modules: inputs z, ext_idx, weights, n_neg, then the K
    prediction tensors [b, W, dim_enc]."""

    @staticmethod
    def forward(ctx, z, ext_idx, weights, n_neg, *preds):
        require_gpu(z, ext_idx, weights, *preds)
        z = f32c(z)
        preds = tuple(f32c(p) for p in preds)
        w = f32c(weights) if weights is not None else None
        losses, acc, saved = _infonce_forward(z, ext_idx, w, n_neg, preds=preds)
        ctx.save_for_backward(z, ext_idx, w, saved, *preds)
        ctx.dims = (z.shape[0], z.shape[1], len(preds), z.shape[2], n_neg)
        ctx.mark_non_differentiable(acc)
        ctx.set_materialize_grads(False)
        return losses, acc

    @staticmethod
    def backward(ctx, dlosses, _dacc):
        lib = _lib.load()
        z, ext_idx, w, saved, *preds = ctx.saved_tensors
        b, t, k, dim_enc, n_neg = ctx.dims
        if dlosses is None:
            dlosses = torch.zeros(k, dtype=torch.float32, device=z.device)
        dlosses = f32c(dlosses)
        dz = torch.empty_like(z)
        dpreds = [torch.empty_like(p) for p in preds]
        sc = scratch(lib.cpc_infonce_scratch_bytes(b, t, k, dim_enc, dim_enc, n_neg), z.device)
        check(lib.cpc_infonce_backward_pred(_lib.ptr_array(preds), ptr(z), ptr(ext_idx), ptr(w), ptr(dlosses), ptr(saved),
                                            ptr(sc), _lib.ptr_array(dpreds), ptr(dz), b, t, k, dim_enc, n_neg,
                                            stream_ptr(z.device)), "infonce_backward_pred")
        return (dz, None, None, None) + tuple(dpreds)


# --------------------------------------------------------------------------- y = x W^T (+ b)
def _rows(x, last_frame):
    """(tensor, byte offset, row stride, rows, width) of the rows a head reads: every frame of x [..., H], or with last_frame
    the frame S - 1 of every sequence of x [B, S, H], read in place (lda = S * H)."""
    if last_frame:
        b, s, h = x.shape
        return x, (s - 1) * h * 4, s * h, b, h
    return x, 0, x.shape[-1], x.numel() // x.shape[-1], x.shape[-1]


def _linear_grads(dy, x, w, dw, db, dx, scale=None, off=0, lda=None):
    """The gradients of y = x W^T + b from dy [m, n] (times the one-element `scale`, in place, when given): db = its column sums
    (cpc_probe_head_backward), dW = dy^T x (cpc_gemm_tn) and, when `dx` is given, dX = dy W (cpc_gemm_nt on the transposed
    weight).  The rows of x and dx start `off` bytes into the tensor and lie `lda` elements apart (_rows)."""
    lib = _lib.load()
    m, n = dy.shape
    kdim = w.shape[1]
    lda = kdim if lda is None else lda
    dev = dy.device
    st = stream_ptr(dev)
    if db is not None:
        nb = lib.cpc_probe_xent_backward_scratch_bytes(n)
        check(lib.cpc_probe_head_backward(ptr(dy), m, n, ptr(scale), ptr(db), ptr(scratch(nb, dev)), nb, st), "probe_head_backward")
    nt = lib.cpc_gemm_tn_scratch_bytes(n, kdim, m)
    check(lib.cpc_gemm_tn(ptr(dy), n, ctypes.c_void_p(x.data_ptr() + off), lda, ptr(dw), kdim, n, kdim, m, ptr(scratch(nt, dev)), nt, st),
          "gemm_tn")
    if dx is not None:
        wt = w.t().contiguous()                                     # [K, N]: the NT form's B operand of dx = dy W
        check(lib.cpc_gemm_nt(ptr(dy), n, ptr(wt), n, ctypes.c_void_p(dx.data_ptr() + off), lda, None, m, kdim, n, st), "gemm_nt")


class _LinearFn(torch.autograd.Function):
    """y = x W^T (+ b) on the library's GEMMs (x [..., K], W [N, K], b [N] or None): the predictions of the linear predictors as
    tensors, for the paths that need them outside the fused kernel (predictor dropout), and the layers of PhoneCriterion."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        require_gpu(x, weight, bias)
        lib = _lib.load()
        x2 = f32c(x).reshape(-1, x.shape[-1])
        w = f32c(weight.detach())
        b = f32c(bias.detach()) if bias is not None else None
        m, kdim = x2.shape
        n = w.shape[0]
        y = torch.empty(m, n, dtype=torch.float32, device=x.device)
        check(lib.cpc_gemm_nt(ptr(x2), kdim, ptr(w), kdim, ptr(y), n, ptr(b), m, n, kdim, stream_ptr(x.device)), "gemm_nt")
        ctx.save_for_backward(x2, w)
        ctx.xshape = x.shape
        ctx.params = (weight, bias)
        return y.view(*x.shape[:-1], n)

    @staticmethod
    def backward(ctx, dy):
        x2, w = ctx.saved_tensors
        dy2 = f32c(dy).reshape(x2.shape[0], w.shape[0])
        dw, db = grad_buffers(ctx.params)
        dx = torch.empty_like(x2)
        _linear_grads(dy2, x2, w, dw, db, dx)
        return dx.view(ctx.xshape), dw, db


# --------------------------------------------------------------------------- modules
class PredictionNetwork(nn.Module):
    """criterion.py:97-173: K predictors under `predictors` (same keys / init as the reference):
    linear (the `else` branch :144-150, nn.Linear(dimOutputAR, dimOutputEncoder, bias=False)), one-layer
    transformers (rnnMode='transformer' :136-143, the fork's default; keys `predictors.{k}.0.*`), or the recurrent
    ones (rnnMode='LSTM' / 'RNN' :115-123)."""

    def __init__(self, nPredicts, dimOutputAR, dimOutputEncoder, rnnMode=None, dropout=False,
                 sizeInputSeq=116, transformer_pruning=0):
        super(PredictionNetwork, self).__init__()
        if rnnMode in ("ffd", "conv4", "conv8", "conv12"):
            raise NotImplementedError(
                f"rnnMode={rnnMode!r}: only 'linear', 'transformer', 'LSTM' and 'RNN' predictors have an MI355X kernel path")
        self.predictors = nn.ModuleList()
        self.RESIDUAL_STD = 0.01
        self.dimOutputAR = dimOutputAR
        # criterion.py:113,168-169: nn.Dropout(0.5) on every prediction in training mode.  The mask comes from torch's
        # generator of the prediction's device (as in the reference's own GPU run: not reproducible against a CPU run)
        self.dropout = nn.Dropout(p=0.5) if dropout else None
        self.rnnMode = rnnMode
        if rnnMode == 'transformer':
            from .transformers import buildTransformerAR
            for _ in range(nPredicts):
                self.predictors.append(buildTransformerAR(dimOutputEncoder, dimOutputAR, nLayers=1,
                                                          sizeSeq=sizeInputSeq, abspos=False))
            return
        if rnnMode in ('LSTM', 'RNN'):                   # criterion.py:115-123
            from .model import LSTMPredictor, RNNPredictor
            for _ in range(nPredicts):
                self.predictors.append(LSTMPredictor(dimOutputAR, dimOutputEncoder, batch_first=True) if rnnMode == 'LSTM'
                                       else RNNPredictor(dimOutputAR, dimOutputEncoder))
            return
        for _ in range(nPredicts):
            self.predictors.append(nn.Linear(dimOutputAR, dimOutputEncoder, bias=False))
            if dimOutputEncoder > dimOutputAR:
                residual = dimOutputEncoder - dimOutputAR
                self.predictors[-1].weight.data.copy_(torch.cat([
                    torch.randn(dimOutputAR, dimOutputAR),
                    self.RESIDUAL_STD * torch.randn(residual, dimOutputAR)], dim=0))

    def packed_weight(self):
        """[K, dimOutputEncoder, dimOutputAR]; autograd splits the gradient back per predictor."""
        return torch.stack([p.weight for p in self.predictors], dim=0)


class MultiHeadPredictionNetwork(nn.Module):
    """criterion.py:44-94 with rnnMode='transformer' (--multihead_rnn): ONE transformer whose feed-forward net emits
    nPredicts residual branches (`predictor.0.*`, a MultiClassifierTransformerHead); prediction k is
    predictor(c)[:, :, k]."""

    def __init__(self, nPredicts, dimOutputAR, dimOutputEncoder, rnnMode='transformer_multi', dropout=False,
                 sizeInputSeq=116, transformer_pruning=0):
        super(MultiHeadPredictionNetwork, self).__init__()
        if rnnMode != 'transformer':
            if rnnMode == 'transformer_adaptive_span':
                raise NotImplementedError("rnnMode='transformer_adaptive_span' is not on the MI355X hot path")
            raise ValueError(f"unknown mode {rnnMode}")
        from .transformers import buildMultHeadTransformerAR
        self.dimOutputAR = dimOutputAR
        self.dropout = nn.Dropout(p=0.5) if dropout else None      # criterion.py:63,86-87
        self.nPredicts = nPredicts
        self.rnnMode = 'transformer_multi'
        self.predictor = buildMultHeadTransformerAR(dimOutputEncoder, dimOutputAR, nLayers=1, sizeSeq=sizeInputSeq,
                                                    abspos=False, nHeads=nPredicts)


class BaseCriterion(nn.Module):

    def warmUp(self):
        return False

    def update(self):
        return


class NoneCriterion(BaseCriterion):
    def __init__(self):
        super(NoneCriterion, self).__init__()

    def forward(self, cFeature, encodedData, label):
        return torch.zeros(1, 1, device=cFeature.device), torch.zeros(1, 1, device=cFeature.device)


class CPCUnsupersivedCriterion(BaseCriterion):
    """criterion.py:193-363."""

    def __init__(self,
                 nPredicts,             # Number of steps
                 dimOutputAR,           # Dimension of G_ar
                 dimOutputEncoder,      # Dimension of the convolutional net
                 negativeSamplingExt,   # Number of negative samples to draw
                 mode=None,
                 rnnMode=False,
                 dropout=False,
                 nSpeakers=0,
                 sizeInputSeq=116,
                 multihead_rnn=False,
                 transformer_pruning=0,
                 n_skipped=0,
                 growth_rate=None,
                 inflection_point_x=None):
        super(CPCUnsupersivedCriterion, self).__init__()
        if multihead_rnn:                                # criterion.py:213-218
            self.wPrediction = MultiHeadPredictionNetwork(nPredicts, dimOutputAR, dimOutputEncoder, rnnMode=rnnMode,
                                                          dropout=dropout, sizeInputSeq=sizeInputSeq - nPredicts,
                                                          transformer_pruning=transformer_pruning)
        else:
            self.wPrediction = PredictionNetwork(nPredicts, dimOutputAR, dimOutputEncoder, rnnMode=rnnMode,
                                                 dropout=dropout, sizeInputSeq=sizeInputSeq - nPredicts)
        self.nSkipped = n_skipped
        self.nPredicts = nPredicts
        self.negativeSamplingExt = negativeSamplingExt
        self.growth_rate = growth_rate
        self.inflection_point_x = inflection_point_x
        self.weighting_function = lambda x: 0.00001 + 1 / (1 + torch.exp(-growth_rate * (x - inflection_point_x)))
        if mode not in [None, "reverse"]:
            raise ValueError("Invalid mode")
        self.mode = mode
        self.sampler = NegativeSampler()
        self._defer_scope = None       # set by deferred_backward() for the duration of the caller's scope

    def seed(self, seed):
        """Use a private negative-index stream (e.g. one per data-parallel rank)."""
        self.sampler.seed(seed)

    def _may_defer(self):
        """No predictor weight with a hook that would read its gradient before the end of the backward pass."""
        for p in self.wPrediction.parameters():
            if getattr(p, "_backward_hooks", None) or getattr(p, "_post_accumulate_grad_hooks", None):
                return False
        return True

    def deferred_backward(self, encoded_full):
        """Context manager: the criterion call(s) inside may run the deferred backward with respect to `encoded_full`, a
        grad_join() output that nothing else consumes (see the comment above join_deferred)."""
        return DeferScope(self, encoded_full)

    def _prepare(self, cFeature, encodedData):
        if self.mode == "reverse":                      # criterion.py:292-294
            encodedData = torch.flip(encodedData, [1])
            cFeature = torch.flip(cFeature, [1])
        return cFeature, encodedData

    def sampleIndices(self, batchSize, nNegativeExt, windowSize, device, time_major=True):
        """Device int32 extIdx (criterion.py:247-266): [batchSize, windowSize, negativeSamplingExt] when
        time_major (the kernels' layout), else the reference's [batchSize, negativeSamplingExt, windowSize]."""
        return self.sampler.sample(batchSize, nNegativeExt, windowSize, self.negativeSamplingExt, device,
                                   time_major=time_major)

    def _predictions(self, cW):
        """The K prediction tensors [b, W, dim_enc] of the predictor modules on cW = c[:, :W] (criterion.py:161-169), or
        None when the predictors are linear and no dropout is active: the fused kernel then computes them itself."""
        net = self.wPrediction
        drop = net.dropout if (net.dropout is not None and self.training) else None
        if net.rnnMode == 'transformer_multi':
            preds = list(torch.unbind(net.predictor(cW), dim=2))            # criterion.py:85 prediction[:, :, k]
        elif net.rnnMode in ('transformer', 'LSTM', 'RNN'):
            preds = [predictor(cW) for predictor in net.predictors]
            preds = [p[0] if isinstance(p, tuple) else p for p in preds]   # criterion.py:164-165
        elif drop is not None:
            preds = [_LinearFn.apply(cW, predictor.weight, None) for predictor in net.predictors]
        else:
            return None
        if drop is not None:
            preds = [drop(p) for p in preds]                                # criterion.py:168-169
        return preds

    def sampleClean(self, encodedData, windowSize):
        """criterion.py:237-286: the K candidate tensors [b, 1 + negativeSamplingExt, windowSize, dimEncoded] (positive first)
        and the all-zero labels.  The negative indices are the reference's, bit for bit (same generator stream, same
        order); the rows are gathered on the device.  The training step never calls this -- its kernel gathers on the
        fly -- it is the reference's inspection API."""
        batchSize, nNegativeExt, dimEncoded = encodedData.size()
        extIdx = self.sampler.sample(batchSize, nNegativeExt, windowSize, self.negativeSamplingExt, encodedData.device,
                                     time_major=False).long()
        rows = encodedData.contiguous().view(-1, dimEncoded)
        negExt = rows.index_select(0, extIdx).view(batchSize, self.negativeSamplingExt, windowSize, dimEncoded)
        labelLoss = torch.zeros(batchSize * windowSize, dtype=torch.long, device=encodedData.device)
        outputs = []
        for k in range(1, self.nPredicts + 1):
            posSeq = encodedData[:, k:k + windowSize].reshape(batchSize, 1, windowSize, dimEncoded)
            outputs.append(torch.cat((posSeq, negExt), dim=1))
        return outputs, labelLoss

    def _logits(self, cFeature, encodedData, extIdx, n_neg):
        """float [b, W, K, 1 + n_neg] straight from the fused forward kernel (no loss, no graph)."""
        lib = _lib.load()
        with torch.no_grad():
            windowSize = cFeature.size(1) - self.nPredicts
            preds = self._predictions(cFeature[:, :windowSize].contiguous())
            z = f32c(encodedData)
            b, t, dim_enc = z.shape
            k = self.nPredicts
            if preds is None:
                dim_ar = cFeature.size(2)
                wpred = torch.stack([f32c(p.weight.detach()) for p in self.wPrediction.predictors], dim=0)
                _losses, _acc, saved = _infonce_forward(z, extIdx, None, n_neg, c=f32c(cFeature), wpred=wpred)
            else:
                dim_ar = dim_enc
                _losses, _acc, saved = _infonce_forward(z, extIdx, None, n_neg, preds=[f32c(p) for p in preds])
            off = lib.cpc_infonce_logits_offset(b, t, k, dim_ar, dim_enc, n_neg)
            n = b * windowSize * k * (n_neg + 1)
            slot_order = saved[off:off + 4 * n].view(torch.float32).view(b, windowSize, k, n_neg + 1)
            # the kernel leaves a (b, t)'s negatives in the order it visited them (sorted by z-row block): back to the caller's
            poff = lib.cpc_infonce_perm_offset(b, t, k, dim_ar, dim_enc, n_neg)
            perm = saved[poff:poff + 2 * b * windowSize * n_neg].view(torch.int16).view(b, windowSize, 1, n_neg).long() & 0xFFFF
            out = torch.empty_like(slot_order)
            out[..., :1] = slot_order[..., :1]
            out[..., 1:].scatter_(3, perm.expand(b, windowSize, k, n_neg), slot_order[..., 1:])
            return out

    def getPrediction(self, cFeature, encodedData, label):
        """criterion.py:291-302: the K score tensors [b, 1 + negativeSamplingExt, W] (candidate 0 = the positive; score =
        mean over channels of prediction * candidate) and the all-zero labels, computed by the fused forward kernel --
        the candidate tensors are not built.  Detached: training goes through forward()."""
        require_gpu(cFeature, encodedData)
        cFeature, encodedData = self._prepare(cFeature, encodedData)
        batchSize, seqSize, _ = cFeature.size()
        windowSize = seqSize - self.nPredicts
        extIdx = self.sampleIndices(batchSize, seqSize, windowSize, cFeature.device)
        logits = self._logits(cFeature, encodedData, extIdx, self.negativeSamplingExt)
        labelLoss = torch.zeros(batchSize * windowSize, dtype=torch.long, device=cFeature.device)
        return [logits[:, :, k].transpose(1, 2).contiguous() for k in range(self.nPredicts)], labelLoss

    def getCosineDistances(self, cFeature, encodedData):
        """criterion.py:304-327: the positive candidate's score alone, K tensors [b, 1, W].  No negative is drawn (the
        generator stream is left untouched): the kernel runs with one dummy negative per position, whose score is dropped."""
        require_gpu(cFeature, encodedData)
        cFeature, encodedData = self._prepare(cFeature, encodedData)
        batchSize, seqSize, _ = cFeature.size()
        windowSize = seqSize - self.nPredicts
        dummy = torch.zeros(batchSize * windowSize, dtype=torch.int32, device=cFeature.device)
        logits = self._logits(cFeature, encodedData, dummy, 1)
        return [logits[:, :, k, :1].transpose(1, 2).contiguous() for k in range(self.nPredicts)]

    def forward(self, cFeature, encodedData, label, signal_quality=None):
        batchSize, seqSize, _ = cFeature.size()
        windowSize = seqSize - self.nPredicts
        cMark, zMark = mark(cFeature), mark(encodedData)
        if cMark is not None and cMark.frames == encodedData.size(1) and seqSize == encodedData.size(1) - self.nPredicts \
                and self.mode != "reverse":
            # the caller (cpcStep) handed over cFeature[:, :windowSize] of a causal context network -- what :296 slices out itself
            seqSize, windowSize = encodedData.size(1), seqSize
        # deferred backward: only inside an explicit deferred_backward() scope of the caller's whose tensor this encodedData is
        # (or is a window slice of: carry_join), and not in reverse mode (the flip is an autograd node of its own that would
        # read dz at once)
        defer = None
        scope = self._defer_scope
        if scope is not None and self.mode != "reverse" and not os.environ.get("CPC_NCE_NO_DEFER") \
                and encodedData.dtype == torch.float32 and encodedData.is_contiguous() and zMark is not None and zMark.join:
            zFull, start = zMark.parent or (encodedData, 0)
            if zFull is scope and self._may_defer():
                defer = (start, batchSize)
        cFeature, encodedData = self._prepare(cFeature, encodedData)
        if signal_quality is not None:                  # criterion.py:334-338
            quality_weighting = self.weighting_function(signal_quality.mean(dim=1))
            quality_weighting = quality_weighting.unsqueeze(1).repeat(1, windowSize).contiguous().view(-1).float()
        else:
            quality_weighting = None                    # ones (criterion.py:340)
        extIdx = self.sampleIndices(batchSize, seqSize, windowSize, cFeature.device)
        preds = self._predictions(cFeature[:, :windowSize].contiguous()) if self._needs_modules() else None
        if preds is not None:
            losses, acc = _InfoNCEPredFn.apply(encodedData, extIdx, quality_weighting, self.negativeSamplingExt, *preds)
        else:
            losses, acc = _InfoNCEFn.apply(cFeature, zFull if defer is not None else encodedData, extIdx, quality_weighting,
                                           self.negativeSamplingExt, defer, *[p.weight for p in self.wPrediction.predictors])
        if self.nSkipped:                              # (a slice of nothing would still cost its backward a zero-fill and a copy)
            losses, acc = losses[self.nSkipped:], acc[self.nSkipped:]
        return losses.view(1, -1), acc.view(1, -1)

    def _needs_modules(self):
        net = self.wPrediction
        return net.rnnMode in ('transformer_multi', 'transformer', 'LSTM', 'RNN') or (net.dropout is not None and self.training)


# --------------------------------------------------------------------------- supervised probe heads (criterion.py:366-538)
class _ProbeHeadFn(torch.autograd.Function):
    """loss of logits = x W^T + b on the library's kernels: cpc_gemm_nt (with the bias) for the logits, then one pass of
    cpc_probe_xent (kind "xent": labels [rows]; returns loss [1] and the accuracy, double [1]) or cpc_probe_ctc (kind "ctc":
    targets [B, maxL] + lengths [B] from collapseLabelChain; the accuracy is 0).  The pass leaves dlogits in place of the
    logits when a gradient is wanted; the backward scales them by the incoming gradient, sums them for db and multiplies them
    out with cpc_gemm_tn (dW) and cpc_gemm_nt (dX)."""

    @staticmethod
    def forward(ctx, x, weight, bias, kind, labels, lengths, last_frame, want_grad):
        require_gpu(x, weight, bias, labels, lengths)
        lib = _lib.load()
        x = f32c(x)
        w = f32c(weight.detach())
        bvec = f32c(bias.detach())
        _, off, lda, n, h = _rows(x, last_frame)
        c = w.shape[0]
        if w.shape[1] != h:
            raise ValueError(f"feature width {h} does not match the classifier's {tuple(w.shape)}")
        dev = x.device
        logits = torch.empty(n, c, dtype=torch.float32, device=dev)
        xp = ctypes.c_void_p(x.data_ptr() + off)
        check(lib.cpc_gemm_nt(xp, lda, ptr(w), h, ptr(logits), c, ptr(bvec), n, c, h, stream_ptr(dev)), "gemm_nt")
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        acc = None
        if kind == "xent":
            labels = labels.reshape(-1).to(torch.int64).contiguous()
            if labels.numel() != n:
                raise ValueError(f"{labels.numel()} labels for {n} rows")
            nll = torch.empty(n, dtype=torch.float32, device=dev)
            correct = torch.empty(n, dtype=torch.int32, device=dev)
            acc = torch.empty(1, dtype=torch.float64, device=dev)
            check(lib.cpc_probe_xent(ptr(logits), ptr(labels), n, c, int(want_grad), ptr(nll), ptr(correct), ptr(loss), ptr(acc),
                                     stream_ptr(dev)), "probe_xent")
        else:
            b, t = x.shape[0], x.shape[1]
            acc = torch.zeros(1, dtype=torch.float32, device=dev)      # (criterion.py:489: avgPER = 0)
            nll = torch.empty(b, dtype=torch.float32, device=dev)
            nb = lib.cpc_probe_ctc_scratch_bytes(b, t, labels.shape[1])
            if nb == 0:
                check(-1, "probe_ctc shape query")
            check(lib.cpc_probe_ctc(ptr(logits), b, t, c, ptr(labels), labels.shape[1], ptr(lengths), ptr(nll), ptr(loss),
                                    ptr(logits) if want_grad else None, ptr(scratch(nb, dev)), nb, stream_ptr(dev)), "probe_ctc")
        ctx.save_for_backward(x, w, logits if want_grad else None)
        ctx.geom = (off, lda, last_frame)
        ctx.params = (weight, bias)
        ctx.mark_non_differentiable(acc)
        return loss, acc

    @staticmethod
    def backward(ctx, dloss, _dacc):
        x, w, dlogits = ctx.saved_tensors
        if dlogits is None:
            raise RuntimeError("the probe head ran without a gradient (want_grad=False) and cannot be differentiated")
        off, lda, last_frame = ctx.geom
        dw, db = grad_buffers(ctx.params)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.zeros_like(x) if last_frame else torch.empty_like(x)
        _linear_grads(dlogits, x, w, dw, db, dx, scale=f32c(dloss.reshape(1)), off=off, lda=lda)
        return dx, dw, db, None, None, None, None, None


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _linear_layers(module):
    """The nn.Linear layers of a classifier (one Linear, or the reference's Sequential(Linear, ReLU, Linear, ...))."""
    return [module] if isinstance(module, nn.Linear) else [m for m in module if isinstance(m, nn.Linear)]


class SpeakerCriterion(BaseCriterion):
    """criterion.py:366-386: a linear classifier on the LAST frame of cFeature (read in place); loss = cross-entropy, acc =
    (argmax == label).double().mean() -- both [1, 1]."""

    def __init__(self, dimEncoder, nSpeakers):
        super(SpeakerCriterion, self).__init__()
        self.linearSpeakerClassifier = nn.Linear(dimEncoder, nSpeakers)

    def forward(self, cFeature, otherEncoded, label):
        lin = self.linearSpeakerClassifier
        loss, acc = _ProbeHeadFn.apply(cFeature, lin.weight, lin.bias, "xent", label, None, True,
                                       _wants_grad(cFeature, lin.weight, lin.bias))
        return loss.view(1, -1), acc.view(1, -1)


class PhoneCriterion(BaseCriterion):
    """criterion.py:418-457: frame-aligned phones; key PhoneCriterionClassifier.{weight,bias} (one layer) or
    PhoneCriterionClassifier.{0,2,...}.* (Linear, ReLU, Linear, ...).  The hidden layers' ReLU is torch.relu; every product and
    the loss head are the library's kernels."""

    def __init__(self, dimEncoder, nPhones, onEncoder, nLayers=1):
        super(PhoneCriterion, self).__init__()
        if nLayers == 1:
            self.PhoneCriterionClassifier = nn.Linear(dimEncoder, nPhones)
        else:
            outLayers = [nn.Linear(dimEncoder, nPhones)]
            for _ in range(nLayers - 1):
                outLayers.append(nn.ReLU())
                outLayers.append(nn.Linear(nPhones, nPhones))
            self.PhoneCriterionClassifier = nn.Sequential(*outLayers)
        self.onEncoder = onEncoder

    def _hidden(self, features):
        """the input of the last Linear: the features themselves, or the hidden layers' output"""
        layers = _linear_layers(self.PhoneCriterionClassifier)
        for lin in layers[:-1]:
            features = torch.relu(_LinearFn.apply(features, lin.weight, lin.bias))
        return features, layers[-1]

    def forward(self, cFeature, otherEncoded, label):
        features = otherEncoded if self.onEncoder else cFeature
        hidden, lin = self._hidden(features)
        loss, acc = _ProbeHeadFn.apply(hidden, lin.weight, lin.bias, "xent", label, None, False,
                                       _wants_grad(hidden, lin.weight, lin.bias))
        return loss.view(1, -1), acc.view(1, -1)

    def getPrediction(self, cFeature):
        hidden, lin = self._hidden(cFeature)
        return _LinearFn.apply(hidden, lin.weight, lin.bias)


class CTCPhoneCriterion(BaseCriterion):
    """criterion.py:460-495: nPhones + 1 outputs (BLANK_LABEL = nPhones), nn.CTCLoss(blank=nPhones, zero_infinity=True) of the
    log-softmax over the S frames, against the collapsed frame labels of every window.  The logged accuracy is 0."""

    def __init__(self, dimEncoder, nPhones, onEncoder):
        super(CTCPhoneCriterion, self).__init__()
        self.PhoneCriterionClassifier = nn.Linear(dimEncoder, nPhones + 1)
        self.onEncoder = onEncoder
        if onEncoder:
            raise ValueError("On encoder version not implemented yet")
        self.BLANK_LABEL = nPhones

    def getPrediction(self, cFeature):
        lin = self.PhoneCriterionClassifier
        return _LinearFn.apply(cFeature, lin.weight, lin.bias)

    def forward(self, cFeature, otherEncoded, label):
        from .seq_alignment import collapse_padded
        lin = self.PhoneCriterionClassifier
        targets, sizes = collapse_padded(label.to(cFeature.device))
        loss, acc = _ProbeHeadFn.apply(cFeature, lin.weight, lin.bias, "ctc", targets, sizes, False,
                                       _wants_grad(cFeature, lin.weight, lin.bias))
        return loss.view(1, -1), acc.view(1, -1)
