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


# ---- the deferred backward (cpc2_hip.h, cpc_infonce_backward with deferred = 1) -----------------------------------------------
# The criterion's dz and predictor weight gradients are produced on a stream of the library's while the context network's
# backward runs; whoever consumes them has to sit behind join_deferred().  Nothing but the caller can promise that, so the
# deferral is an EXPLICIT opt-in of the caller's, never something a tensor attribute switches on by travelling through
# wrappers: `with criterion.deferred_backward(encoded_full): criterion(c, z, label)` (cpcStep does it) states that
#   * `encoded_full` came out of grad_join() (CPCModel.forward applies it BEFORE the context network, so autograd runs its
#     backward after the context network's and before anything that reads the summed gradient of the encoder output),
#   * the criterion call inside the scope is the ONLY consumer of that tensor (a second loss term on it, or a tensor hook,
#     would make autograd read dz before the join), and
#   * nothing reads the predictors' weight gradients before the backward pass has ended.
# The scope is refused (the backward then runs at once, on the caller's stream) when the criterion object is not the bare
# module (DistributedDataParallel / DataParallel around it: DDP's reducer copies a weight gradient into its bucket the moment
# autograd accumulates it, i.e. before the side stream has written it) or when a predictor weight carries a backward or
# post-accumulate hook.  A callback at the end of the backward pass joins whatever is still pending (an encoder without
# gradient: nobody reads dz, the optimiser reads the weight gradients).
_deferred = {}          # device index -> tensors the side stream still reads / writes (kept alive until the join)


def join_deferred(device):
    """Make the current stream of `device` wait for a pending deferred criterion backward (no-op when none is)."""
    device = torch.device(device)
    if device.type != "cuda":
        return
    if _deferred.pop(_lib.device_index(device), None) is not None:
        check(_lib.load().cpc_infonce_join(stream_ptr(device)), "infonce_join")


class _GradJoin(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        join_deferred(g.device)
        return g


def grad_join(encoded):
    """Identity on the encoder output; its backward is where a deferred criterion backward is joined.  Returns the tensor the
    criterion should be given (marked `_cpc_join`; `_cpc_join_source` = the tensor whose gradient is the complete one)."""
    if not (encoded.is_cuda and encoded.requires_grad and torch.is_grad_enabled()):
        return encoded
    out = _GradJoin.apply(encoded)
    out._cpc_join = True
    out._cpc_join_source = encoded
    return out


def carry_join(view, parent, start):
    """`view` = parent[start:start + n] (windows) of a grad_join() output.  The criterion then differentiates with respect to
    `parent` itself (its dz lands in rows start.. of a gradient of parent's size), so that no slicing node of autograd's --
    which would read dz BEFORE the context network's backward, i.e. before the join -- sits between the two."""
    if getattr(parent, "_cpc_join", False) and parent.is_contiguous() and view.is_contiguous() and \
            view.data_ptr() == parent.data_ptr() + start * parent.stride(0) * parent.element_size():
        view._cpc_join = True
        view._cpc_join_parent = (parent, int(start))
    return view


# ---- gradients that are zero by construction, without materialising the zeros every step ----------------------------------------
# train.py:102-103 slices the model's outputs (context of the first b windows, targets of the last b): autograd turns each slice's
# gradient back into the full tensor with a zero fill plus a copy (16.8 MB + 8.4 MB per slice at the benchmark shape, two small
# launches each).  The halves that are zero are zero EVERY step, so they live in buffers that are allocated and zeroed once per
# (device, shape, slot): the criterion's backward writes dc / dz straight into the other half and hands the whole buffer on.
# Nothing ever writes the zero half (autograd only reads gradients it does not own: this cache holds a reference), and a buffer is
# reused only after the backward pass that read it has been enqueued on the same stream.
from ._tail import _cached_grad_buffer, grad_home, grad_home_view  # noqa: E402


class _FirstWindows(torch.autograd.Function):
    """x[:n] (windows) whose backward does not fill and copy: the gradient of the slice is written by its producer straight into
    the first n windows of a cached buffer whose other windows stay zero (see above); any other gradient is copied into it."""

    @staticmethod
    def forward(ctx, x, n):
        ctx.full_shape, ctx.n = tuple(x.shape), n
        out = x[:n]
        return out.view_as(out)

    @staticmethod
    def backward(ctx, g):
        buf = _cached_grad_buffer(ctx.full_shape, g.device, ("context", ctx.n))
        if not (g.data_ptr() == buf.data_ptr() and g.is_contiguous() and g.dtype == torch.float32):
            buf[:ctx.n].copy_(g)
        return buf, None


def first_windows(x, n):
    """x[:n] for the context features in cpcStep (train.py:102); marks the result so that the criterion's backward writes its
    gradient where _FirstWindows.backward expects it."""
    if not (x.is_cuda and x.requires_grad and torch.is_grad_enabled() and x.is_contiguous() and x.dtype == torch.float32):
        return x[:n]
    out = _FirstWindows.apply(x, n)
    out._cpc_first_of = (tuple(x.shape), n)
    return out


class _SplitWindows(torch.autograd.Function):
    """(x[:n], x[n:]) along the window axis whose backward neither fills nor adds: both gradients are written by their producers
    straight into the two parts of ONE cached buffer (grad_home), which is handed on whole.  The deferred criterion backward is
    joined here -- autograd runs this node when BOTH gradients are due, i.e. after the context network's backward."""

    @staticmethod
    def forward(ctx, x, n, tag):
        ctx.full_shape, ctx.n, ctx.tag = tuple(x.shape), n, tag
        ctx.set_materialize_grads(False)
        first, rest = x[:n], x[n:]
        return first.view_as(first), rest.view_as(rest)

    @staticmethod
    def backward(ctx, g_first, g_rest):
        n = ctx.n
        device = (g_first if g_first is not None else g_rest).device
        join_deferred(device)
        buf = _cached_grad_buffer(ctx.full_shape, device, (ctx.tag, n))
        row = buf.stride(0) * buf.element_size()
        for g, part, at in ((g_first, buf[:n], 0), (g_rest, buf[n:], n)):
            if g is None:
                part.zero_()
            elif not (g.data_ptr() == buf.data_ptr() + at * row and g.is_contiguous() and g.dtype == torch.float32):
                part.copy_(g)
        return buf, None, None


def split_windows(x, n, tag="split"):
    """cpcStep's split of the encoder output [2b, T, H] into the context network's windows x[:n] and the criterion's target windows
    x[n:] (train.py:99-103 keeps exactly these: the context of the first half, the encoded data of the second).  Each part is marked
    with its home in the gradient buffer (`_cpc_grad_home`, honoured by the recurrent / transformer / criterion backward) and the
    second with `_cpc_join`: whoever consumes the gradient of `x` sits behind the join of a deferred criterion backward."""
    if not (x.is_cuda and x.requires_grad and torch.is_grad_enabled() and x.is_contiguous() and x.dtype == torch.float32):
        return x[:n], x[n:]
    first, rest = _SplitWindows.apply(x, n, tag)
    first._cpc_grad_home = (tuple(x.shape), (tag, n), 0)
    rest._cpc_grad_home = (tuple(x.shape), (tag, n), n)
    rest._cpc_join = True
    return first, rest


class _FirstFrames(torch.autograd.Function):
    """x[:, :w] (the frames the criterion uses) as a contiguous tensor; the gradient goes back into x's home in the gradient buffer
    (grad_home), whose frames w.. nobody writes: they stay zero from the buffer's allocation on (its slot is this form's own)."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.home, ctx.shape, ctx.w = grad_home(x), tuple(x.shape), w
        return x[:, :w].contiguous()

    @staticmethod
    def backward(ctx, g):
        if ctx.home is not None:
            full_shape, slot, start = ctx.home
            buf = _cached_grad_buffer(full_shape, g.device, slot)[start:start + ctx.shape[0]]
        else:
            buf = torch.zeros(ctx.shape, dtype=torch.float32, device=g.device)
        buf[:, :ctx.w].copy_(g)
        return buf, None


def first_frames(x, w, total):
    """x[:, :w] of a `total`-frame sequence for a causal context network whose later frames nobody uses (criterion.py:296 keeps
    cFeature[:, :windowSize]); the result is marked `_cpc_frames_of = total` so that the criterion knows it was handed the slice."""
    if x.is_cuda and x.requires_grad and torch.is_grad_enabled() and x.dtype == torch.float32 and x.is_contiguous():
        out = _FirstFrames.apply(x, w)
    else:
        out = x[:, :w].contiguous()
    out._cpc_frames_of = total
    return out


class _DeferScope:
    def __init__(self, criterion, encoded_full):
        self.criterion, self.tensor = criterion, encoded_full

    def __enter__(self):
        ok = getattr(self.tensor, "_cpc_join", False) and not hasattr(self.tensor, "_cpc_join_parent")
        self.criterion._defer_scope = self.tensor if ok else None
        return self

    def __exit__(self, *exc):
        self.criterion._defer_scope = None
        return False


class _InfoNCEFn(torch.autograd.Function):
    """inputs: c, z, ext_idx, weights, n_neg, defer, then the K predictor weights [dim_enc, dim_ar].  defer: None, or
    (start, n): the criterion's targets are windows start .. start + n of z and the backward is the deferred one."""

    @staticmethod
    def forward(ctx, c, z, ext_idx, weights, n_neg, defer, *wk):
        require_gpu(c, z, ext_idx, weights, *wk)
        lib = _lib.load()
        ctx.c_first_of = getattr(c, "_cpc_first_of", None) if (c.is_contiguous() and c.dtype == torch.float32) else None
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
        b, tc, dim_ar = c.shape
        k, dim_enc, _ = wpred.shape
        t = z.shape[1]
        # c holds the t frames of the sequence, or only the W = t - k the criterion uses (criterion.py:296: cFeature[:, :windowSize])
        if z.shape != (b, t, dim_enc) or wpred.shape[2] != dim_ar or tc not in (t, t - k):
            raise ValueError(f"shape mismatch c={tuple(c.shape)} z={tuple(z.shape)} W={tuple(wpred.shape)}")
        if ext_idx.dtype != torch.int32 or ext_idx.numel() != b * n_neg * (t - k):
            raise ValueError("ext_idx must be int32 [b, W, n_neg]")
        if weights is not None and weights.numel() != b * (t - k):
            raise ValueError(f"weights must hold one value per (window, frame): {b * (t - k)}, got {weights.numel()}")
        w = f32c(weights) if weights is not None else None
        nsaved = lib.cpc_infonce_saved_bytes(b, t, k, dim_ar, dim_enc, n_neg)
        nscratch = lib.cpc_infonce_scratch_bytes(b, t, k, dim_ar, dim_enc, n_neg)
        if nsaved == 0:
            check(-1, "infonce shape query")
        losses = torch.empty(k, dtype=torch.float32, device=c.device)
        acc = torch.empty(k, dtype=torch.float32, device=c.device)
        saved = torch.empty(nsaved, dtype=torch.uint8, device=c.device)
        sc = scratch(nscratch, c.device)
        check(lib.cpc_infonce_forward(ptr(c), ptr(z), ptr(wpred), ptr(ext_idx), ptr(w), ptr(losses), ptr(acc),
                                      ptr(saved), ptr(sc), b, t, tc, k, dim_ar, dim_enc, n_neg, stream_ptr(c.device)), "infonce_forward")
        ctx.save_for_backward(c, z, wpred, ext_idx, w, saved)
        ctx.param_refs = wk
        ctx.dims = (b, t, k, dim_ar, dim_enc, n_neg)
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
        if ctx.c_first_of is not None:       # (first_windows: dc goes where the slice's backward looks for it, the rest stays zero)
            dc = _cached_grad_buffer(ctx.c_first_of[0], c.device, ("context", ctx.c_first_of[1]))[:c.shape[0]]
        else:
            dc = torch.empty_like(c)
        defer = ctx.z_full_shape is not None
        if defer and ctx.z_full_shape != tuple(z.shape):
            # (windows outside start .. start + n get no gradient from the criterion: zero once, see _cached_grad_buffer)
            dz_out = _cached_grad_buffer(ctx.z_full_shape, z.device, ("targets", ctx.z_start, z.shape[0]))
            dz = dz_out[ctx.z_start:ctx.z_start + z.shape[0]]
        else:
            dz_out = dz = grad_home_view(ctx.z_home, z)
        gw = grad_buffers(ctx.param_refs)
        dw = _packed_view(gw)                 # contiguous in the flat gradient buffer -> written in place
        direct = dw is not None
        if not direct:
            dw = torch.empty_like(wpred)
        nscratch = lib.cpc_infonce_scratch_bytes(b, t, k, dim_ar, dim_enc, n_neg)
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
            _deferred[_lib.device_index(c.device)] = (c, z, wpred, ext_idx, w, dlosses, saved, sc, dz_out, dw)
            device = c.device
            torch.autograd.Variable._execution_engine.queue_callback(lambda: join_deferred(device))
        if not direct:
            gw = list(dw.unbind(0))
        return (dc, dz_out, None, None, None, None) + tuple(gw)


class _InfoNCEPredFn(torch.autograd.Function):
    """Same criterion, predictions supplied by predictor modules: inputs z, ext_idx, weights, n_neg, then the K
    prediction tensors [b, W, dim_enc]."""

    @staticmethod
    def forward(ctx, z, ext_idx, weights, n_neg, *preds):
        require_gpu(z, ext_idx, weights, *preds)
        lib = _lib.load()
        z = f32c(z)
        preds = tuple(f32c(p) for p in preds)
        b, t, dim_enc = z.shape
        k = len(preds)
        if any(p.shape != (b, t - k, dim_enc) for p in preds):
            raise ValueError(f"predictions must be [b, W, dim_enc] = {(b, t - k, dim_enc)}")
        if ext_idx.dtype != torch.int32 or ext_idx.numel() != b * n_neg * (t - k):
            raise ValueError("ext_idx must be int32 [b, W, n_neg]")
        if weights is not None and weights.numel() != b * (t - k):
            raise ValueError(f"weights must hold one value per (window, frame): {b * (t - k)}, got {weights.numel()}")
        w = f32c(weights) if weights is not None else None
        nsaved = lib.cpc_infonce_saved_bytes(b, t, k, dim_enc, dim_enc, n_neg)
        nscratch = lib.cpc_infonce_scratch_bytes(b, t, k, dim_enc, dim_enc, n_neg)
        if nsaved == 0:
            check(-1, "infonce shape query")
        losses = torch.empty(k, dtype=torch.float32, device=z.device)
        acc = torch.empty(k, dtype=torch.float32, device=z.device)
        saved = torch.empty(nsaved, dtype=torch.uint8, device=z.device)
        sc = scratch(nscratch, z.device)
        check(lib.cpc_infonce_forward_pred(_lib.ptr_array(preds), ptr(z), ptr(ext_idx), ptr(w), ptr(losses), ptr(acc),
                                           ptr(saved), ptr(sc), b, t, k, dim_enc, n_neg, stream_ptr(z.device)),
              "infonce_forward_pred")
        ctx.save_for_backward(z, ext_idx, w, saved, *preds)
        ctx.dims = (b, t, k, dim_enc, n_neg)
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


class _LinearFn(torch.autograd.Function):
    """y = x W^T on the library's GEMMs (x [..., K], W [N, K]): the predictions of the linear predictors as tensors, for the
    paths that need them outside the fused kernel (predictor dropout)."""

    @staticmethod
    def forward(ctx, x, weight):
        require_gpu(x, weight)
        lib = _lib.load()
        x2 = f32c(x).reshape(-1, x.shape[-1])
        w = f32c(weight.detach())
        m, kdim = x2.shape
        n = w.shape[0]
        y = torch.empty(m, n, dtype=torch.float32, device=x.device)
        check(lib.cpc_gemm_nt(ptr(x2), kdim, ptr(w), kdim, ptr(y), n, None, m, n, kdim, stream_ptr(x.device)), "gemm_nt")
        ctx.save_for_backward(x2, w)
        ctx.xshape = x.shape
        return y.view(*x.shape[:-1], n)

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x2, w = ctx.saved_tensors
        m, kdim = x2.shape
        n = w.shape[0]
        dy2 = f32c(dy).reshape(m, n)
        wt = w.t().contiguous()                                     # [K, N]: the NT form's B operand of dx = dy W
        dx = torch.empty(m, kdim, dtype=torch.float32, device=dy.device)
        check(lib.cpc_gemm_nt(ptr(dy2), n, ptr(wt), n, ptr(dx), kdim, None, m, kdim, n, stream_ptr(dy.device)), "gemm_nt")
        dw = torch.empty(n, kdim, dtype=torch.float32, device=dy.device)
        nb = lib.cpc_gemm_tn_scratch_bytes(n, kdim, m)
        sc = scratch(nb, dy.device)
        check(lib.cpc_gemm_tn(ptr(dy2), n, ptr(x2), kdim, ptr(dw), kdim, n, kdim, m, ptr(sc), nb, stream_ptr(dy.device)), "gemm_tn")
        return dx.view(ctx.xshape), dw


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
        return _DeferScope(self, encoded_full)

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
            preds = [_LinearFn.apply(cW, predictor.weight) for predictor in net.predictors]
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
            losses = torch.empty(k, dtype=torch.float32, device=z.device)
            acc = torch.empty(k, dtype=torch.float32, device=z.device)
            dim_ar = dim_enc if preds is not None else cFeature.size(2)
            nsaved = lib.cpc_infonce_saved_bytes(b, t, k, dim_ar, dim_enc, n_neg)
            if nsaved == 0:
                check(-1, "infonce shape query")
            saved = torch.empty(nsaved, dtype=torch.uint8, device=z.device)
            sc = scratch(lib.cpc_infonce_scratch_bytes(b, t, k, dim_ar, dim_enc, n_neg), z.device)
            if preds is None:
                c = f32c(cFeature)
                wpred = torch.stack([f32c(p.weight.detach()) for p in self.wPrediction.predictors], dim=0)
                check(lib.cpc_infonce_forward(ptr(c), ptr(z), ptr(wpred), ptr(extIdx), None, ptr(losses), ptr(acc), ptr(saved),
                                              ptr(sc), b, t, t, k, dim_ar, dim_enc, n_neg, stream_ptr(z.device)), "infonce_forward")
            else:
                preds = [f32c(p) for p in preds]
                check(lib.cpc_infonce_forward_pred(_lib.ptr_array(preds), ptr(z), ptr(extIdx), None, ptr(losses), ptr(acc),
                                                   ptr(saved), ptr(sc), b, t, k, dim_enc, n_neg, stream_ptr(z.device)),
                      "infonce_forward_pred")
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
        if getattr(cFeature, "_cpc_frames_of", None) == encodedData.size(1) and seqSize == encodedData.size(1) - self.nPredicts \
                and self.mode != "reverse":
            # the caller (cpcStep) handed over cFeature[:, :windowSize] of a causal context network -- what :296 slices out itself
            seqSize, windowSize = encodedData.size(1), seqSize
        # deferred backward: only inside an explicit deferred_backward() scope of the caller's whose tensor this encodedData is
        # (or is a window slice of: carry_join), and not in reverse mode (the flip is an autograd node of its own that would
        # read dz at once)
        defer = None
        scope = self._defer_scope
        if scope is not None and self.mode != "reverse" and not os.environ.get("CPC_NCE_NO_DEFER") \
                and encodedData.dtype == torch.float32 and encodedData.is_contiguous() and getattr(encodedData, "_cpc_join", False):
            zFull, start = getattr(encodedData, "_cpc_join_parent", (encodedData, 0))
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
def _rows(x, last_frame):
    """(tensor, byte offset, row stride, rows, width) of the rows a head reads: every frame of x [..., H], or with last_frame
    the frame S - 1 of every sequence of x [B, S, H], read in place (lda = S * H)."""
    if last_frame:
        b, s, h = x.shape
        return x, (s - 1) * h * 4, s * h, b, h
    return x, 0, x.shape[-1], x.numel() // x.shape[-1], x.shape[-1]


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
        ctx.geom = (off, lda, n, h, c, last_frame)
        ctx.params = (weight, bias)
        ctx.mark_non_differentiable(acc)
        return loss, acc

    @staticmethod
    def backward(ctx, dloss, _dacc):
        lib = _lib.load()
        x, w, dlogits = ctx.saved_tensors
        if dlogits is None:
            raise RuntimeError("the probe head ran without a gradient (want_grad=False) and cannot be differentiated")
        off, lda, n, h, c, last_frame = ctx.geom
        dev = x.device
        st = stream_ptr(dev)
        dw, db = grad_buffers(ctx.params)
        nb = lib.cpc_probe_xent_backward_scratch_bytes(c)
        check(lib.cpc_probe_head_backward(ptr(dlogits), n, c, ptr(f32c(dloss.reshape(1))), ptr(db), ptr(scratch(nb, dev)), nb, st),
              "probe_head_backward")
        xp = ctypes.c_void_p(x.data_ptr() + off)
        nt = lib.cpc_gemm_tn_scratch_bytes(c, h, n)
        check(lib.cpc_gemm_tn(ptr(dlogits), c, xp, lda, ptr(dw), h, c, h, n, ptr(scratch(nt, dev)), nt, st), "gemm_tn")
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.zeros_like(x) if last_frame else torch.empty_like(x)
            wt = w.t().contiguous()                                     # [H, C]: the NT form's B operand of dx = dlogits W
            check(lib.cpc_gemm_nt(ptr(dlogits), c, ptr(wt), c, ctypes.c_void_p(dx.data_ptr() + off), lda, None, n, h, c, st),
                  "gemm_nt")
        return dx, dw, db, None, None, None, None, None


class _AffineFn(torch.autograd.Function):
    """y = x W^T + b on the library's GEMMs (the hidden layers of PhoneCriterion with nLayers > 1)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        require_gpu(x, weight, bias)
        lib = _lib.load()
        x2 = f32c(x).reshape(-1, x.shape[-1])
        w = f32c(weight.detach())
        m, k = x2.shape
        n = w.shape[0]
        y = torch.empty(m, n, dtype=torch.float32, device=x.device)
        check(lib.cpc_gemm_nt(ptr(x2), k, ptr(w), k, ptr(y), n, ptr(f32c(bias.detach())), m, n, k, stream_ptr(x.device)), "gemm_nt")
        ctx.save_for_backward(x2, w)
        ctx.xshape = x.shape
        ctx.params = (weight, bias)
        return y.view(*x.shape[:-1], n)

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x2, w = ctx.saved_tensors
        m, k = x2.shape
        n = w.shape[0]
        dev = dy.device
        st = stream_ptr(dev)
        dy2 = f32c(dy).reshape(m, n)
        dw, db = grad_buffers(ctx.params)
        nb = lib.cpc_probe_xent_backward_scratch_bytes(n)
        check(lib.cpc_probe_head_backward(ptr(dy2), m, n, None, ptr(db), ptr(scratch(nb, dev)), nb, st), "probe_head_backward")
        nt = lib.cpc_gemm_tn_scratch_bytes(n, k, m)
        check(lib.cpc_gemm_tn(ptr(dy2), n, ptr(x2), k, ptr(dw), k, n, k, m, ptr(scratch(nt, dev)), nt, st), "gemm_tn")
        dx = torch.empty(m, k, dtype=torch.float32, device=dev)
        wt = w.t().contiguous()
        check(lib.cpc_gemm_nt(ptr(dy2), n, ptr(wt), n, ptr(dx), k, None, m, k, n, st), "gemm_nt")
        return dx.view(ctx.xshape), dw, db


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
            features = torch.relu(_AffineFn.apply(features, lin.weight, lin.bias))
        return features, layers[-1]

    def forward(self, cFeature, otherEncoded, label):
        features = otherEncoded if self.onEncoder else cFeature
        hidden, lin = self._hidden(features)
        loss, acc = _ProbeHeadFn.apply(hidden, lin.weight, lin.bias, "xent", label, None, False,
                                       _wants_grad(hidden, lin.weight, lin.bias))
        return loss.view(1, -1), acc.view(1, -1)

    def getPrediction(self, cFeature):
        hidden, lin = self._hidden(cFeature)
        return _AffineFn.apply(hidden, lin.weight, lin.bias)


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
        return _AffineFn.apply(cFeature, lin.weight, lin.bias)

    def forward(self, cFeature, otherEncoded, label):
        from .seq_alignment import collapse_padded
        lin = self.PhoneCriterionClassifier
        targets, sizes = collapse_padded(label.to(cFeature.device))
        loss, acc = _ProbeHeadFn.apply(cFeature, lin.weight, lin.bias, "ctc", targets, sizes, False,
                                       _wants_grad(cFeature, lin.weight, lin.bias))
        return loss.view(1, -1), acc.view(1, -1)
