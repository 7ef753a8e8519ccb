"""Gradient routing of cpcStep: where the gradients of the step's activations are written (cached buffers with a fixed layout,
handed on without a fill, a copy or an add) and where a criterion backward that was left on the library's side stream is joined
(cpc2_hip.h: cpc_infonce_backward with deferred = 1, cpc_infonce_join).  The autograd Functions of model.py, transformers.py and
criterion.py and cpcStep itself (train.py) share it; it depends on none of them."""
from dataclasses import dataclass

import torch

from . import _lib
from ._lib import check, stream_ptr


# --------------------------------------------------------------------------- the mark on an activation tensor
@dataclass
class Mark:
    """What this module knows about a tensor it handed out (ONE attribute, `_cpc_mark`; only this module touches it)."""
    join: bool = False          # whoever consumes this tensor's gradient sits behind join_deferred() (grad_join, split_windows)
    source: object = None       # grad_join: the tensor whose gradient is the complete one
    parent: object = None       # carry_join: (parent, start) -- this tensor is windows start.. of that grad_join() output
    home: object = None         # (full_shape, slot, start): the gradient's fixed place in a cached buffer (grad_home)
    claimed: bool = False       # a consumer has taken the home: the next one gets a buffer of its own
    frames: object = None       # mark_frames: the output of a context network that ran on the first frames of this many


def mark(t):
    """The Mark of `t`, or None."""
    return getattr(t, "_cpc_mark", None)


def _marked(t, **fields):
    t._cpc_mark = Mark(**fields)
    return t


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


def keep_deferred(device, tensors):
    """A deferred criterion backward has just been launched on `device`: `tensors` stay alive until it is joined, at the end of
    the backward pass at the latest."""
    _deferred[_lib.device_index(device)] = tensors
    torch.autograd.Variable._execution_engine.queue_callback(lambda: join_deferred(device))


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
    criterion should be given (marked `join`; `source` = the tensor whose gradient is the complete one)."""
    if not (encoded.is_cuda and encoded.requires_grad and torch.is_grad_enabled()):
        return encoded
    return _marked(_GradJoin.apply(encoded), join=True, source=encoded)


def carry_join(view, parent, start):
    """`view` = parent[start:start + n] (windows) of a grad_join() output.  The criterion then differentiates with respect to
    `parent` itself (its dz lands in rows start.. of a gradient of parent's size), so that no slicing node of autograd's --
    which would read dz BEFORE the context network's backward, i.e. before the join -- sits between the two."""
    m = mark(parent)
    if m is not None and m.join and parent.is_contiguous() and view.is_contiguous() and \
            view.data_ptr() == parent.data_ptr() + start * parent.stride(0) * parent.element_size():
        _marked(view, join=True, parent=(parent, int(start)))
    return view


class DeferScope:
    """`with criterion.deferred_backward(encoded_full):` -- see above.  Sets criterion._defer_scope to the tensor for the duration
    of the scope when that tensor is a grad_join() / split_windows() output itself (not a carry_join view of one)."""

    def __init__(self, criterion, encoded_full):
        self.criterion, self.tensor = criterion, encoded_full

    def __enter__(self):
        m = mark(self.tensor)
        ok = m is not None and m.join and m.parent is None
        self.criterion._defer_scope = self.tensor if ok else None
        return self

    def __exit__(self, *exc):
        self.criterion._defer_scope = None
        return False


# --------------------------------------------------------------------------- gradients with a fixed home
# Buffers for gradients whose layout is fixed by the caller (the zero halves of train.py:102-103's slices; cpcStep's split of the
# encoder output into context windows and target windows): allocated and zeroed once per (shape, device, slot), the
# producers write their part in place and the consumer hands the whole buffer on.  A buffer is reused only after the backward pass
# that read it has been enqueued on the same stream; the slot carries every number the "stays zero" / "who writes what" invariant
# depends on (window counts), so two users with the same full shape but different splits never share one.
_grad_cache = {}


def cached_grad_buffer(shape, device, slot):
    key = (tuple(shape), str(device), slot)
    buf = _grad_cache.get(key)
    if buf is None:
        if len(_grad_cache) > 8:
            _grad_cache.clear()
        buf = _grad_cache[key] = torch.zeros(shape, dtype=torch.float32, device=device)
    return buf


def grad_home(t):
    """(full_shape, slot, start) a tensor was marked with by split_windows / first_windows, if it can be honoured: the gradient with
    respect to `t` should be written into windows start.. of that cached buffer -- the consumer then takes it without a copy."""
    m = mark(t)
    if m is None or m.home is None or not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        return None
    # ONE consumer per home: a second function that takes the same tagged tensor would write the same memory, and autograd would
    # then add the buffer to itself (twice the last gradient, no error).  The first forward that honours the home claims it.
    if m.claimed:
        return None
    full_shape, _slot, start = m.home
    if tuple(t.shape[1:]) != tuple(full_shape[1:]) or start + t.shape[0] > full_shape[0]:
        return None
    m.claimed = True
    return m.home


def grad_home_view(home, like):
    """The piece of its home buffer a gradient shaped like `like` is written into (None: no home, allocate)."""
    if home is None:
        return torch.empty_like(like)
    full_shape, slot, start = home
    return cached_grad_buffer(full_shape, like.device, slot)[start:start + like.shape[0]]


# ---- gradients that are zero by construction, without materialising the zeros every step ----------------------------------------
# train.py:102-103 slices the model's outputs (context of the first b windows, targets of the last b): autograd turns each slice's
# gradient back into the full tensor with a zero fill plus a copy (16.8 MB + 8.4 MB per slice at the benchmark shape, two small
# launches each).  The halves that are zero are zero EVERY step, so they live in buffers that are allocated and zeroed once per
# (device, shape, slot): the criterion's backward writes dc / dz straight into the other half and hands the whole buffer on.
# Nothing ever writes the zero half (autograd only reads gradients it does not own: this cache holds a reference), and a buffer is
# reused only after the backward pass that read it has been enqueued on the same stream.
def _routable(x):
    return x.is_cuda and x.requires_grad and torch.is_grad_enabled() and x.is_contiguous() and x.dtype == torch.float32


def _is_piece(g, buf, at):
    """The gradient `g` already IS windows at.. of `buf` (its producer honoured the home)."""
    return g.data_ptr() == buf.data_ptr() + at * buf.stride(0) * buf.element_size() and g.is_contiguous() and g.dtype == torch.float32


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
        buf = cached_grad_buffer(ctx.full_shape, g.device, ("context", ctx.n))
        if not _is_piece(g, buf, 0):
            buf[:ctx.n].copy_(g)
        return buf, None


def first_windows(x, n):
    """x[:n] for the context features in cpcStep (train.py:102); marks the result with its home in the gradient buffer, so that the
    criterion's backward writes its gradient where _FirstWindows.backward expects it."""
    if not _routable(x):
        return x[:n]
    return _marked(_FirstWindows.apply(x, n), home=(tuple(x.shape), ("context", n), 0))


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
        buf = cached_grad_buffer(ctx.full_shape, device, (ctx.tag, n))
        for g, part, at in ((g_first, buf[:n], 0), (g_rest, buf[n:], n)):
            if g is None:
                part.zero_()
            elif not _is_piece(g, buf, at):
                part.copy_(g)
        return buf, None, None


def split_windows(x, n, tag="split"):
    """cpcStep's split of the encoder output [2b, T, H] into the context network's windows x[:n] and the criterion's target windows
    x[n:] (train.py:99-103 keeps exactly these: the context of the first half, the encoded data of the second).  Each part is marked
    with its home in the gradient buffer (`home`, honoured by the recurrent / transformer / criterion backward) and the
    second with `join`: whoever consumes the gradient of `x` sits behind the join of a deferred criterion backward."""
    if not _routable(x):
        return x[:n], x[n:]
    first, rest = _SplitWindows.apply(x, n, tag)
    shape, slot = tuple(x.shape), (tag, n)
    return _marked(first, home=(shape, slot, 0)), _marked(rest, home=(shape, slot, n), join=True)


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
            buf = cached_grad_buffer(full_shape, g.device, slot)[start:start + ctx.shape[0]]
        else:
            buf = torch.zeros(ctx.shape, dtype=torch.float32, device=g.device)
        buf[:, :ctx.w].copy_(g)
        return buf, None


def first_frames(x, w):
    """x[:, :w] for a causal context network whose later frames nobody uses (criterion.py:296 keeps cFeature[:, :windowSize]).  The
    network's output is then marked with mark_frames()."""
    if _routable(x):
        return _FirstFrames.apply(x, w)
    return x[:, :w].contiguous()


def mark_frames(c_feature, total):
    """`c_feature` is the output of a causal context network on first_frames() of a `total`-frame sequence (`frames = total`), so
    that the criterion knows it was handed cFeature[:, :windowSize]."""
    return _marked(c_feature, frames=total)
