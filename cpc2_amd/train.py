"""The caller side of the hot path: factories, the optimisation step, data-parallel glue and the training command line
(`python -m cpc2_amd.train`, the reference's cpc/train.py: parseArgs / main at the end of this file).

Mirrors (semantics, names) /root/reference/cpc/train.py:27-59 (getCriterion), :72-187
(trainStep / valStep), :472-484 (Adam over criterion + model parameters), :523-527 (DDP wrap) and
/root/reference/cpc/feature_loader.py:202-235 (getEncoder / getAR).  Differences, all deliberate:
  * device-agnostic tensors come from the caller (the reference hard-codes .cuda());
  * parameters and gradients live in ONE flat fp32 buffer each, so the optimiser is one fused
    HIP Adam launch and data parallelism is one RCCL all-reduce per step (instead of DDP buckets);
  * per-step losses stay on the device; the host reads them every `loggingStep` steps only.
"""
import copy
import json
import time

import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from ._lib import check, ptr, stream_ptr
from ._route import carry_join, first_frames, first_windows, mark, mark_frames, split_windows
from .criterion import CPCUnsupersivedCriterion, NoneCriterion
from .model import CPCAR, CPCEncoder, CPCModel, join_tail


# --------------------------------------------------------------------------- factories
def getEncoder(args):
    """feature_loader.py:202-212 (CPCEncoder branch)."""
    if getattr(args, "encoder_type", "cpc") in ("mfcc", "lfb"):
        raise NotImplementedError("only the raw-waveform CPCEncoder is on the MI355X hot path")
    return CPCEncoder(args.hiddenEncoder, args.normMode)


def getAR(args):
    """feature_loader.py:215-235: every branch (transformer, the bidirectional GRU of cpc_mode='bert', no_ar, CPCAR)."""
    if args.arMode == "transformer":
        from .transformers import buildTransformerAR
        arNet = buildTransformerAR(args.hiddenEncoder, args.hiddenGar, args.nLevelsGRU,
                                   args.sizeWindow // 160, args.abspos)
        args.hiddenGar = args.hiddenEncoder
        return arNet
    if getattr(args, "cpc_mode", None) == "bert":
        from .model import BiDIRARTangled
        return BiDIRARTangled(args.hiddenEncoder, args.hiddenGar, args.nLevelsGRU)
    if args.arMode == "no_ar":
        from .model import NoAr
        return NoAr()
    return CPCAR(args.hiddenEncoder, args.hiddenGar, args.samplingType == "sequential", args.nLevelsGRU,
                 mode=args.arMode, reverse=getattr(args, "cpc_mode", None) == "reverse")


def getCriterion(args, downsampling, nSpeakers=0, nPhones=0):
    """train.py:27-48 (unsupervised branch)."""
    if getattr(args, "supervised", False):
        raise NotImplementedError("--supervised: the supervised criteria are not trained through this loop (in the reference this path fails at the first step); train them with python -m cpc2_amd.eval.linear_separability --unfrozen")
    if getattr(args, "cpc_mode", None) == "none":
        return NoneCriterion()
    sizeInputSeq = args.sizeWindow // downsampling
    return CPCUnsupersivedCriterion(args.nPredicts, args.hiddenGar, args.hiddenEncoder, args.negativeSamplingExt,
                                    mode=getattr(args, "cpc_mode", None), rnnMode=args.rnnMode,
                                    dropout=getattr(args, "dropout", False), nSpeakers=nSpeakers,
                                    sizeInputSeq=sizeInputSeq,
                                    multihead_rnn=getattr(args, "multihead_rnn", False),
                                    transformer_pruning=getattr(args, "transformer_pruning", 0),
                                    n_skipped=getattr(args, "n_skipped", 0),
                                    growth_rate=getattr(args, "growth_rate", None),
                                    inflection_point_x=getattr(args, "inflection_point_x", None))


# --------------------------------------------------------------------------- flat parameters + fused Adam / SGD
class _FlatOptimizer(torch.optim.Optimizer):
    """What FlatAdam and FlatSGD share: every parameter re-homed into `self.flat` (views, same values), every .grad into
    `self.flat_grad`, ONE param group (so the reference's schedulers attach unchanged: the learning rate is read from
    param_groups[0]["lr"] at every step), and the bookkeeping DataParallelContext and run() rely on."""

    def _rehome(self, params, defaults, direct_grads):
        self.params = [p for p in params]
        self.direct_grads = direct_grads
        if not self.params:
            raise ValueError(f"{type(self).__name__} got an empty parameter list")
        dev = self.params[0].device
        _lib.require_gpu(*self.params)
        torch.optim.Optimizer.__init__(self, self.params, defaults)
        self.step_count = 0
        total = sum(p.numel() for p in self.params)
        self.flat = torch.empty(total, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros(total, dtype=torch.float32, device=dev)
        self.offsets = []
        off = 0
        for p in self.params:
            n = p.numel()
            self.flat[off:off + n].copy_(p.data.reshape(-1))
            p.data = self.flat[off:off + n].view(p.shape)
            if direct_grads:
                # the fused backward kernels write each gradient straight into flat_grad and autograd adopts
                # that view as .grad (no per-parameter add kernels); see _lib.grad_buffers
                p._cpc_flat = (self.flat_grad, off)
                p.grad = None
            else:
                p.grad = self.flat_grad[off:off + n].view(p.shape)
            self.offsets.append(off)
            off += n
        return total, dev

    def zero_grad(self, set_to_none=False):
        self.flat_grad.zero_()
        if self.direct_grads:
            for p in self.params:
                p.grad = None
            return
        for p, off in zip(self.params, self.offsets):      # re-attach if someone replaced .grad
            if p.grad is None or p.grad.data_ptr() != self.flat_grad.data_ptr() + 4 * off:
                p.grad = self.flat_grad[off:off + p.numel()].view(p.shape)

    def _gather_stray_grads(self, ranges=None):
        """direct mode: a gradient that autograd did NOT adopt from flat_grad (accumulated or produced by a
        torch op) lives in its own tensor: copy it home before the fused update.  ranges: only the parameters inside
        these [lo, hi) pieces of the flat buffer (the others have been all-reduced already)."""
        base = self.flat_grad.data_ptr()
        for p, off in zip(self.params, self.offsets):
            if ranges is not None and not any(lo <= off < hi for lo, hi in ranges):
                continue
            if p.grad is not None and p.grad.data_ptr() != base + 4 * off:
                self.flat_grad[off:off + p.numel()].copy_(p.grad.reshape(-1))

    def _before_step(self, closure):
        if closure is not None:
            raise NotImplementedError(f"{type(self).__name__}.step does not re-evaluate a closure")
        if self.flat.is_cuda:
            join_tail(self.flat.device)          # (a deferred recurrent backward's weight gradients: normally joined at the end of backward)
        if self.direct_grads:
            self._gather_stray_grads()
        self.step_count += 1
        return self.param_groups[0]["lr"]

    def _group_state(self, **hyper):
        """The param group of a state dict.  `initial_lr` (written into the group by a torch scheduler) travels with it: a
        scheduler built on a resumed optimiser takes its base rate from there, and from the CURRENT -- already scaled -- rate
        when it is missing (a run stopped inside the warm-up ramp would ramp from the scaled rate)."""
        group = dict(lr=self.param_groups[0]["lr"], **hyper)
        if "initial_lr" in self.param_groups[0]:
            group["initial_lr"] = self.param_groups[0]["initial_lr"]
        group["params"] = list(range(len(self.params)))
        return group

    def _load_group(self, sd):
        group = sd["param_groups"][0]
        self.param_groups[0]["lr"] = group["lr"]
        if "initial_lr" in group:
            self.param_groups[0]["initial_lr"] = group["initial_lr"]


class FlatAdam(_FlatOptimizer):
    """torch.optim.Adam(params, lr, betas, eps) of train.py:477-479 on one flat buffer.

    Re-homes every parameter into `self.flat` (views, same values) and every .grad into
    `self.flat_grad`, then `step()` is a single cpc_adam_step launch.  State-dict interop with
    torch.optim.Adam is kept through `state_dict()` / `load_state_dict()` (per-parameter
    exp_avg / exp_avg_sq / step).  A torch.optim.Optimizer with ONE param group, so the reference's
    learning-rate schedulers (train.py:501-520: StepLR, the LambdaLR ramp, SchedulerCombiner) attach
    to it unchanged; the learning rate is read from param_groups[0]["lr"] at every step."""

    def __init__(self, params, lr=2e-4, betas=(0.9, 0.999), eps=1e-8, direct_grads=True):
        total, dev = self._rehome(params, dict(lr=lr, betas=betas, eps=eps), direct_grads)
        self.lr, self.betas, self.eps = lr, betas, eps
        self.exp_avg = torch.zeros(total, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(total, dtype=torch.float32, device=dev)

    def step(self, closure=None, grad_scale=1.0):
        lr = self._before_step(closure)
        check(_lib.load().cpc_adam_step(ptr(self.flat), ptr(self.flat_grad), ptr(self.exp_avg), ptr(self.exp_avg_sq),
                                        self.flat.numel(), self.step_count, lr, self.betas[0], self.betas[1], self.eps,
                                        grad_scale, stream_ptr(self.flat.device)), "adam_step")

    def state_dict(self):
        state = {}
        for i, (p, off) in enumerate(zip(self.params, self.offsets)):
            n = p.numel()
            state[i] = {"step": torch.tensor(float(self.step_count)),
                        "exp_avg": self.exp_avg[off:off + n].view(p.shape).clone(),
                        "exp_avg_sq": self.exp_avg_sq[off:off + n].view(p.shape).clone()}
        return {"state": state, "param_groups": [self._group_state(betas=self.betas, eps=self.eps)]}

    def load_state_dict(self, sd):
        for i, (p, off) in enumerate(zip(self.params, self.offsets)):
            st = sd["state"].get(i)
            if st is None:
                continue
            n = p.numel()
            self.exp_avg[off:off + n].copy_(st["exp_avg"].reshape(-1))
            self.exp_avg_sq[off:off + n].copy_(st["exp_avg_sq"].reshape(-1))
            self.step_count = int(st["step"])
        self._load_group(sd)


class FlatSGD(_FlatOptimizer):
    """torch.optim.SGD(params, lr, momentum=0.9) of train.py:480-482 on one flat buffer: `step()` is a single cpc_sgd_step
    launch over (flat, flat_grad, momentum_buffer) -- the first step copies the gradient into the buffer, the following ones
    compute buf = momentum buf + g, and p -= lr buf.  Same non-finite-gradient rule as FlatAdam (element left alone,
    asynchronous error reported).  `state_dict()` / `load_state_dict()` use torch.optim.SGD's layout (`momentum_buffer` per
    parameter, no entry before the first step)."""

    def __init__(self, params, lr=2e-4, momentum=0.9, direct_grads=True):
        total, dev = self._rehome(params, dict(lr=lr, momentum=momentum), direct_grads)
        self.lr, self.momentum = lr, momentum
        self.momentum_buffer = torch.zeros(total, dtype=torch.float32, device=dev)

    def step(self, closure=None, grad_scale=1.0):
        lr = self._before_step(closure)
        check(_lib.load().cpc_sgd_step(ptr(self.flat), ptr(self.flat_grad), ptr(self.momentum_buffer), self.flat.numel(),
                                       self.step_count, lr, self.momentum, grad_scale, stream_ptr(self.flat.device)), "sgd_step")

    def state_dict(self):
        state = {}
        if self.step_count > 0:
            for i, (p, off) in enumerate(zip(self.params, self.offsets)):
                state[i] = {"momentum_buffer": self.momentum_buffer[off:off + p.numel()].view(p.shape).clone()}
        group = self._group_state(momentum=self.momentum, dampening=0, weight_decay=0, nesterov=False, maximize=False,
                                  foreach=None, differentiable=False, fused=None)
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        """A parameter without a buffer in `sd` gets a zero one, which the next step treats as torch does a missing one
        (momentum x 0 + g = g); with no buffer at all the next step is a first step."""
        self.momentum_buffer.zero_()
        self.step_count = 0
        for i, (p, off) in enumerate(zip(self.params, self.offsets)):
            buf = (sd["state"].get(i) or {}).get("momentum_buffer")
            if buf is not None:
                self.momentum_buffer[off:off + p.numel()].copy_(buf.reshape(-1))
                self.step_count = 1
        self._load_group(sd)


def buildOptimizer(cpcModel, cpcCriterion, lr=2e-4, beta1=0.9, beta2=0.999, epsilon=1e-8, optimizer='adam'):
    """train.py:472-484: criterion parameters first, then model parameters; 'adam' or 'sgd' (momentum 0.9)."""
    g_params = list(cpcCriterion.parameters()) + list(cpcModel.parameters())
    if optimizer == 'adam':
        return FlatAdam(g_params, lr=lr, betas=(beta1, beta2), eps=epsilon)
    if optimizer == 'sgd':
        return FlatSGD(g_params, lr=lr, momentum=0.9)
    raise ValueError("Unsupported optimizer: %s" % optimizer)


# --------------------------------------------------------------------------- logs (cpc/utils/misc.py:25-60)
def save_logs(data, pathLogs):
    with open(pathLogs, 'w') as file:
        json.dump(data, file, indent=2)


def update_logs(logs, logStep, prevlogs=None):
    """Every entry (minus prevlogs') divided by logStep.  The callers pass the LAST batch index, i.e. the number of batches
    minus 1: with one batch numpy divides by zero (inf / nan and a warning, no exception), as in the reference."""
    out = {}
    for key in logs:
        out[key] = copy.deepcopy(logs[key])
        if prevlogs is not None:
            out[key] -= prevlogs[key]
        out[key] /= logStep
    return out


def show_logs(text, logs):
    print("")
    print('-' * 50)
    print(text)
    for key in logs:
        if key == "iter":
            continue
        nPredicts = logs[key].shape[0]
        strSteps = ['Step'] + [str(s) for s in range(1, nPredicts + 1)]
        formatCommand = ' '.join(['{:>16}' for x in range(nPredicts + 1)])
        print(formatCommand.format(*strSteps))
        strLog = [key] + ["{:10.6f}".format(s) for s in logs[key]]
        print(formatCommand.format(*strLog))
    print('-' * 50)


# --------------------------------------------------------------------------- learning-rate schedule
def ramp_scheduling_function(n_epoch_ramp, epoch, square_ramp=False):
    """cpc/utils/misc.py:77-83: linear (or squared) warm-up factor over the first n_epoch_ramp epochs."""
    if epoch >= n_epoch_ramp:
        return 1
    frac = (epoch + 1) / n_epoch_ramp
    return frac ** 2 if square_ramp else frac


class SchedulerCombiner:
    """cpc/utils/misc.py:85-122: schedulers activated one after the other.  step() advances every scheduler from the
    one before the current activation boundary on, LAST first -- so while the ramp is active the step schedule's
    epoch counter already runs, and the ramp (stepped last) has the final word on the learning rate."""

    def __init__(self, scheduler_list, activation_step, curr_step=0):
        if len(scheduler_list) != len(activation_step):
            raise ValueError("The number of scheduler must be the same as the number of activation step")
        if activation_step[0] > curr_step:
            raise ValueError("The first activation step cannot be higher than the current step.")
        self.scheduler_list = scheduler_list
        self.activation_step = list(activation_step)
        self.curr_step = curr_step

    def step(self):
        import bisect
        self.curr_step += 1
        first = bisect.bisect_left(self.activation_step, self.curr_step) - 1
        for i in reversed(range(first, len(self.scheduler_list))):
            self.scheduler_list[i].step()

    def __str__(self):
        return "SchedulerCombiner \n(\n" + "".join(f"({i}) {sc} \n" for i, sc in enumerate(self.scheduler_list)) + ")\n"


def buildScheduler(optimizer, schedulerStep=-1, schedulerRamp=None, epochs_done=0):
    """train.py:501-520: StepLR(gamma 0.5) every schedulerStep epochs, a linear ramp over the first schedulerRamp
    epochs, both (combined), or None; then fast-forwarded over the epochs a resumed run has behind it."""
    scheduler = None
    if schedulerStep > 0:
        scheduler = torch.optim.lr_scheduler.StepLR(optimizer, schedulerStep, gamma=0.5)
    if schedulerRamp is not None:
        n_epoch = schedulerRamp
        ramp = torch.optim.lr_scheduler.LambdaLR(optimizer, lr_lambda=lambda epoch: ramp_scheduling_function(n_epoch, epoch),
                                                 last_epoch=-1)
        scheduler = ramp if scheduler is None else SchedulerCombiner([ramp, scheduler], [0, schedulerRamp])
    if scheduler is not None:
        for _ in range(epochs_done):
            scheduler.step()
    return scheduler


# --------------------------------------------------------------------------- data parallel
class DataParallelContext:
    """One process per GPU (train.py:291-295, 523-527 with --distributed).  Replaces the two DDP wrappers by: one
    broadcast of the flat parameter buffer from rank 0 at start, and all-reduces (SUM) of the flat gradient buffer whose
    1/world_size is folded into the optimiser's kernel (Adam or SGD).

    Overlap (the reference gets it from DDP's buckets, train.py:523-527): with `early_params` -- the parameters whose
    gradients are complete before the encoder's backward starts: the criterion's and the context network's -- their slices
    of the flat gradient are reduced ASYNCHRONOUSLY from an autograd hook on the encoder's output (`attach`, called by
    cpcStep), i.e. while the encoder's backward kernels run; `reduce_and_step` then reduces the encoder's slice, waits
    for the early ones and updates.  Without early_params (or overlap=False): one blocking all-reduce of the whole buffer.
    `DataParallelContext.for_modules(optimizer, cpcModel, cpcCriterion)` takes the early parameters from the modules.

    ONE backward pass per optimisation step: the hook reduces the early slices at the end of the first backward pass
    after `attach`; a second backward pass before `reduce_and_step` (gradient accumulation) would add onto sums.  `attach`
    raises if it is called again before `reduce_and_step` has consumed a fired hook.

    `trace`: None, or a callable(kind, lo, hi, view) invoked on the compute stream right before every all-reduce
    ("pre": view = flat_grad[lo:hi] as this rank computed it) and after the last one of a step ("post": the whole
    buffer of sums) -- the equivalence tests clone what they see there (tests/dp_job.py)."""

    def __init__(self, optimizer, early_params=None, overlap=True, trace=None, timing=False):
        self.opt = optimizer
        self.trace = trace
        self.timing = timing                    # bench.py: events around the part of a step the exchange holds the stream for
        self._spans = []
        self._coop_seen = None
        self._helper = None                     # the stream the early all-reduces are issued from (attach)
        self.active = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size() if self.active else 1
        self.early, self.late, self._pending, self._fired = [], [], [], False
        if self.active:
            dist.broadcast(self.opt.flat, src=0)
            if early_params and overlap and hasattr(optimizer, "offsets"):
                self._split(early_params)

    @classmethod
    def for_modules(cls, optimizer, cpcModel, cpcCriterion, overlap=True, trace=None):
        """The context the training loop uses: the criterion's and the context network's parameters reduce early."""
        inner = getattr(cpcModel, "module", cpcModel)
        crit = getattr(cpcCriterion, "module", cpcCriterion)
        early = list(crit.parameters()) + (list(inner.gAR.parameters()) if hasattr(inner, "gAR") else [])
        return cls(optimizer, early_params=early, overlap=overlap, trace=trace)

    def _split(self, early_params):
        """[lo, hi) ranges of the flat buffer: early (merged runs of the early parameters) and the rest."""
        ids = {id(p) for p in early_params}
        total = self.opt.flat.numel()
        marks = sorted((off, off + p.numel()) for p, off in zip(self.opt.params, self.opt.offsets) if id(p) in ids)
        for lo, hi in marks:
            if self.early and self.early[-1][1] == lo:
                self.early[-1] = (self.early[-1][0], hi)
            else:
                self.early.append((lo, hi))
        pos = 0
        for lo, hi in self.early:
            if lo > pos:
                self.late.append((pos, lo))
            pos = hi
        if pos < total:
            self.late.append((pos, total))

    def _all_reduce(self, lo, hi, async_op=False):
        """SUM over the ranks of flat_grad[lo:hi], in place, enqueued behind everything the current stream holds."""
        view = self.opt.flat_grad[lo:hi]
        if self.trace is not None:
            self.trace("pre", lo, hi, view)
        return dist.all_reduce(view, op=dist.ReduceOp.SUM, async_op=async_op)

    # ---- what the exchange costs a step (bench.py's `comm.exposed_ms_per_step`)
    def timing_reset(self):
        self._spans = []

    def timing_read(self):
        """Mean milliseconds per reduce_and_step() during which the compute stream was held by the exchange (from the start of
        the late all-reduce to the end of the waits for the early ones), or None without a process group / timing."""
        if not (self.active and self.timing and self._spans):
            return None
        torch.cuda.synchronize()
        return sum(a.elapsed_time(b) for a, b in self._spans) / len(self._spans)

    def _span(self):
        if not (self.timing and self.opt.flat_grad.is_cuda):
            return None
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    @staticmethod
    def _coop_launches():
        """Cooperative recurrent launches of this process so far (cpc2_hip.h, cpc_coop_launches)."""
        return int(_lib.load().cpc_coop_launches())

    def attach(self, encoder_output):
        """Register the hook that starts the early reductions when the gradient of `encoder_output` is ready (everything
        downstream of the encoder has then written its parameter gradients)."""
        m = mark(encoder_output)
        if m is not None and m.source is not None:              # (_route.py, grad_join)
            encoder_output = m.source
        if not (self.active and self.early and encoder_output.requires_grad):
            return
        if self._fired:
            raise RuntimeError("DataParallelContext: a backward pass has already reduced the early gradient slices of this "
                               "step; call reduce_and_step() before the next forward pass (one backward pass per step)")
        # Cooperative recurrent kernels (GRU / LSTM at hidden 256 / 512) need EVERY workgroup resident; a collective's kernels
        # share the device.  The schedule keeps the two apart by stream order: the early all-reduce is issued behind the recurrent
        # backward (it waits for everything the compute stream holds at that point), and reduce_and_step() makes the compute
        # stream wait for every collective before the next step's forward pass.  The first half is asserted here: if the forward
        # pass of this step launched cooperative kernels, a recurrent backward (cooperative or not: the two fit a CU separately)
        # must have been issued before the hook fires.
        on_gpu = self.opt.flat_grad.is_cuda
        now = self._coop_launches() if on_gpu else 0
        fwd_coop = now - (self._coop_seen if self._coop_seen is not None else now)
        bwd_calls_at_attach = int(_lib.load().cpc_recurrent_backward_calls()) if on_gpu else 0

        def start(_grad):
            if not self._fired:                 # once per backward pass
                self._fired = True
                if on_gpu and fwd_coop > 0 and int(_lib.load().cpc_recurrent_backward_calls()) == bwd_calls_at_attach:
                    raise RuntimeError("DataParallelContext: the early all-reduce would be issued BEFORE the recurrent backward of "
                                       "this step (a collective's kernels beside a cooperative kernel that needs every workgroup "
                                       "resident): attach() must be given the encoder output, upstream of the context network")
                if getattr(self.opt, "direct_grads", False):
                    self.opt._gather_stray_grads(self.early)     # a gradient autograd did not write in place (accumulation)
                if not on_gpu:
                    self._pending = [self._all_reduce(lo, hi, async_op=True) for lo, hi in self.early]
                    return
                # The early slices are complete once the compute stream has reached this point AND the library's side stream has
                # finished the context network's deferred weight gradients.  Only the EXCHANGE has to wait for the latter: it is issued
                # from a helper stream that is ordered behind both, and the compute stream goes straight on into the encoder's
                # backward (round 4 joined the side stream into the compute stream here: ~0.1 ms of the encoder's backward waiting
                # for products nothing in it reads).  The deferred calls' buffers stay on the books until the join at the end of the
                # backward pass / in reduce_and_step().
                device = self.opt.flat_grad.device
                if self._helper is None:
                    # (a stream of the library's making: on a hardware queue that is neither the compute stream's nor the side
                    #  stream's -- a pool stream that happened to share the compute stream's queue would park the wait for the side
                    #  stream IN FRONT of the encoder's backward; cpc2_hip.h, cpc_stream_create_apart)
                    import ctypes
                    raw = ctypes.c_void_p()
                    avoid = (ctypes.c_void_p * 1)(torch.cuda.current_stream(device).cuda_stream)
                    check(_lib.load().cpc_stream_create_apart(avoid, 1, ctypes.byref(raw)), "stream_create_apart")
                    self._helper = torch.cuda.ExternalStream(raw.value, device=device)
                self._helper.wait_stream(torch.cuda.current_stream(device))
                with torch.cuda.stream(self._helper):
                    check(_lib.load().cpc_side_tail_wait(stream_ptr(device)), "side_tail_wait")
                    self._pending = [self._all_reduce(lo, hi, async_op=True) for lo, hi in self.early]
        encoder_output.register_hook(start)

    def reduce_and_step(self):
        if self.opt.flat_grad.is_cuda:
            join_tail(self.opt.flat_grad.device)                 # (parameter gradients still on the library's side stream)
        if self.active and self.opt.flat_grad.is_cuda:
            self._coop_seen = self._coop_launches()              # (the next step's forward launches count from here)
        if self.active:
            if self._fired and self._pending:
                if getattr(self.opt, "direct_grads", False):
                    self.opt._gather_stray_grads(self.late)      # (the early slices hold SUMS by now)
                t0 = self._span()
                for lo, hi in self.late:
                    self._all_reduce(lo, hi)
                with _lib.host_wait("collective_wait"):
                    for work in self._pending:
                        work.wait()
                if t0 is not None:
                    self._spans.append((t0, self._span()))
                if self.trace is not None:
                    self.trace("post", 0, self.opt.flat_grad.numel(), self.opt.flat_grad)
                # the optimiser must not take a stray early gradient for the reduced one again
                stray = getattr(self.opt, "direct_grads", False)
                if stray:
                    self.opt.direct_grads = False
                try:
                    self.opt.step(grad_scale=1.0 / self.world)
                finally:
                    if stray:
                        self.opt.direct_grads = True
                self._pending, self._fired = [], False
                return
            if getattr(self.opt, "direct_grads", False):
                self.opt._gather_stray_grads()
            t0 = self._span()
            self._all_reduce(0, self.opt.flat_grad.numel())
            if t0 is not None:
                self._spans.append((t0, self._span()))
            if self.trace is not None:
                self.trace("post", 0, self.opt.flat_grad.numel(), self.opt.flat_grad)
            self._pending, self._fired = [], False
        self.opt.step(grad_scale=1.0 / self.world)


# --------------------------------------------------------------------------- the step
def _context_windows_only(cpcModel):
    """May cpcStep run the context network on the b context windows alone?  train.py:99-103 keeps `c_feature[:b]` and
    `encoded_data[b:]` of the model's 2b-window outputs: the context of the future half is sliced away, its gradient is identically
    zero and so are its terms in every parameter gradient.  Every context network of this package is per window (no statistics
    across windows), so running it on the first b windows gives the same c_feature[:b], the same gradients and the same update.
    Only for the bare CPCModel (a wrapper's forward() is the plug-in boundary and stays the 2b-window call), without span masking
    (its numpy draws cover all 2b rows) and without a state carried across calls (keepHidden stores the hidden state of all
    2b windows)."""
    import os
    from .model import BiDIRAR, BiDIRARTangled, NoAr
    from .transformers import StaticPositionEmbedding, TransformerLayer
    if os.environ.get("CPC_STRICT_2B") or type(cpcModel) is not CPCModel or cpcModel.mask_prob > 0.0:
        return False
    if not hasattr(cpcModel.gEncoder, "forward_channel_last"):
        return False
    # this form calls gEncoder.forward_channel_last and gAR directly: forward (pre-)hooks registered on the model or its encoder
    # (feature taps, profilers) would silently stop firing -- with hooks the reference's own call is kept
    for m in (cpcModel, cpcModel.gEncoder):
        if m._forward_hooks or m._forward_pre_hooks:
            return False
    ar = cpcModel.gAR
    if isinstance(ar, CPCAR):
        return not ar.keepHidden and ar.hidden is None
    if isinstance(ar, (NoAr, BiDIRAR, BiDIRARTangled)):
        return True
    return isinstance(ar, torch.nn.Sequential) and all(isinstance(m, (StaticPositionEmbedding, TransformerLayer)) for m in ar)


def _guard_cooperative_kernels(cpcModel, cpcCriterion):
    """The cooperative recurrent kernels (GRU / LSTM at hidden 256 / 512) need every workgroup resident, i.e. nothing else on the
    CUs while they run.  DataParallelContext keeps its collectives away from them by stream order; the reference's arrangement --
    DistributedDataParallel (or DataParallel over several devices) around model / criterion, train.py:523-532 -- does not: DDP
    all-reduces the criterion's bucket (an RCCL kernel on the same CUs) while the recurrent backward runs.  Handed such a wrapper
    on an RCCL process group, the process switches to the streaming recurrent kernels for good (cpc_coop_set_policy)."""
    wrappers = (torch.nn.parallel.DistributedDataParallel, torch.nn.DataParallel)
    if not (isinstance(cpcModel, wrappers) or isinstance(cpcCriterion, wrappers)):
        return
    multi_dp = any(isinstance(m, torch.nn.DataParallel) and len(m.device_ids or ()) > 1 for m in (cpcModel, cpcCriterion))
    on_rccl = dist.is_available() and dist.is_initialized() and dist.get_backend() == "nccl"
    if (multi_dp or on_rccl) and _lib.load().cpc_coop_set_policy(-1) == 0:
        _lib.load().cpc_coop_set_policy(1)


def _context_frames_only(cpcModel, cpcCriterion, frames):
    """May the context network stop after the W = frames - nPredicts steps whose output the criterion reads?  criterion.py:296 keeps
    `cFeature[:, :windowSize]`; a context network that is CAUSAL in time (the recurrent ones, forward direction) and keeps no state
    across calls computes those W frames without the nPredicts behind them, and their gradient is identically zero -- the same
    argument as for the context windows, on the time axis.  Returns W, or 0."""
    import os
    if os.environ.get("CPC_STRICT_FRAMES") or type(cpcCriterion) is not CPCUnsupersivedCriterion or cpcCriterion.mode == "reverse":
        return 0
    ar = cpcModel.gAR
    if not isinstance(ar, CPCAR) or ar.reverse or ar.keepHidden or ar.hidden is not None:
        return 0
    w = frames - cpcCriterion.nPredicts
    return w if w >= 1 else 0


def cpcStep(past, future, label, cpcModel, cpcCriterion, signal_quality=None, dedup=False, dp=None, strict=False):
    """train.py:95-108: model on cat([past, future]); context from the past half, targets from the
    future half; returns (totLoss, allLosses [1,K], allAcc [1,K]).

    Default: the encoder runs on the 2b windows, the context network on the b windows whose context the reference keeps
    (_context_windows_only: identical outputs, gradients and updates).  strict=True: the reference's own dataflow, the
    context network on all 2b windows through CPCModel.forward.

    dedup=True: when `future` IS `past` (no augmentation: dataset.py:308-321 yields the same window twice) the
    two halves of the reference's 2b-window batch are identical and every op up to the criterion is per
    window, so one pass over b windows gives bit-identical c_feature / encoded_data at half the work."""
    b = past.size(0)
    if past.is_cuda:
        _guard_cooperative_kernels(cpcModel, cpcCriterion)
    if dedup and (future is past or (future.data_ptr() == past.data_ptr() and future.shape == past.shape)):
        with _ar_scope(cpcModel):
            c_feature, encoded_data, label = cpcModel(past, label)
        if dp is not None:
            dp.attach(encoded_data)
        with _defer_scope(cpcCriterion, encoded_data):
            allLosses, allAcc = cpcCriterion(c_feature, encoded_data, label, signal_quality)
        return sum_losses(allLosses), allLosses, allAcc
    if not strict and _context_windows_only(cpcModel):
        with _ar_scope(cpcModel):
            # (train.py:99's cat([past, future]) as two pointers: only the first layer reads the waveform)
            encoded_full = cpcModel.gEncoder.forward_channel_last(past, future)      # [2b, T, H]
            frames = encoded_full.size(1)
            w = _context_frames_only(cpcModel, cpcCriterion, frames)
            if w:
                # ... and only over the W frames criterion.py:296 keeps of it (a causal recurrent network: _context_frames_only)
                context_in, encoded_data = split_windows(encoded_full, b, tag=("split_w", w))
                c_feature = mark_frames(cpcModel.gAR(first_frames(context_in, w)), frames)      # [b, W, H]
            else:
                context_in, encoded_data = split_windows(encoded_full, b)
                c_feature = cpcModel.gAR(context_in)                                  # [b, T, H]: train.py:102's c_feature[:b]
        if dp is not None:
            dp.attach(encoded_full)
        with _defer_scope(cpcCriterion, encoded_data):
            allLosses, allAcc = cpcCriterion(c_feature, encoded_data, label, signal_quality)
        return sum_losses(allLosses), allLosses, allAcc
    combined = torch.cat([past, future], dim=0)
    # (train.py:100,105 concatenate the labels too and take the first half back: CPCModel hands `label` through untouched, so the
    #  round trip -- two small kernels per step -- is skipped for it; any other model gets the reference's tensors)
    passthrough = isinstance(getattr(cpcModel, "module", cpcModel), CPCModel)
    with _ar_scope(cpcModel):
        c_feature, encoded_full, label2 = cpcModel(combined, label if passthrough else torch.cat([label, label]))
    label = label2 if passthrough else label2[:b]
    if dp is not None:
        dp.attach(encoded_full)             # data parallel: the criterion / context gradients are reduced under the encoder's backward
    c_feature = first_windows(c_feature, b)
    encoded_data = carry_join(encoded_full[b:, :, :], encoded_full, b)
    with _defer_scope(cpcCriterion, encoded_full):
        allLosses, allAcc = cpcCriterion(c_feature, encoded_data, label, signal_quality)
    return sum_losses(allLosses), allLosses, allAcc


# ---- totLoss = allLosses.sum(); totLoss.backward() without the four one-element kernels autograd puts between the criterion's
# forward and backward kernels (ones_like of the root, the sum's expand, the copy that makes it contiguous: ~30 us of a 5 ms step)
_ONES = {}


def _ones(device, n):
    key = (str(device), n)
    t = _ONES.get(key)
    if t is None:
        t = _ONES[key] = torch.ones(n, dtype=torch.float32, device=device)
    return t


class _SumLosses(torch.autograd.Function):
    """x.sum() whose backward hands out a cached tensor of ones when the incoming gradient is backward()'s cached 1.0."""

    @staticmethod
    def forward(ctx, x):
        ctx.shape = x.shape
        return x.sum()

    @staticmethod
    def backward(ctx, g):
        n = 1
        for d in ctx.shape:
            n *= d
        if g.data_ptr() == _ones(g.device, 1).data_ptr():
            return _ones(g.device, n).view(ctx.shape)
        return g.expand(ctx.shape)


def sum_losses(allLosses):
    """train.py:106 (`totLoss = allLosses.sum()`)."""
    if allLosses.is_cuda and allLosses.dtype == torch.float32 and allLosses.requires_grad:
        return _SumLosses.apply(allLosses)
    return allLosses.sum()


def backward(totLoss):
    """train.py:109 (`totLoss.backward()`), seeded with a cached 1.0 instead of a fresh ones_like."""
    if totLoss.is_cuda and totLoss.dtype == torch.float32 and totLoss.dim() == 0:
        totLoss.backward(gradient=_ones(totLoss.device, 1).view(()))
    else:
        totLoss.backward()


def _ar_scope(cpcModel):
    """The context network's and the encoder's deferred parameter gradients (model.py, deferred_weight_gradients) are cpcStep's to
    allow for the BARE model only: the gradients are read by the optimiser after the backward pass (and by DataParallelContext's early
    all-reduce, which joins first) -- a DistributedDataParallel / DataParallel wrapper would read them as they are accumulated."""
    import contextlib
    stack = contextlib.ExitStack()
    if isinstance(cpcModel, CPCModel):
        for m in cpcModel.modules():            # CPCEncoder, CPCAR, TransformerLayer
            if hasattr(m, "deferred_weight_gradients"):
                stack.enter_context(m.deferred_weight_gradients())
    return stack


def _defer_scope(cpcCriterion, encoded_full):
    """The criterion's deferred backward (criterion.py, deferred_backward) is this function's to allow: the encoder output
    never leaves cpcStep, so the criterion call is its only consumer.  Only for the bare criterion module -- wrapped the way
    the reference wraps it (DistributedDataParallel, train.py:526; DataParallel, :531) the wrapper's reducer reads the
    predictors' weight gradients as soon as autograd has accumulated them, before a side stream could have written them."""
    import contextlib
    if isinstance(cpcCriterion, CPCUnsupersivedCriterion):
        return cpcCriterion.deferred_backward(encoded_full)
    return contextlib.nullcontext()


def _check_async(device):
    """Raise if a cooperative recurrent kernel timed out since the last check (it then produced NaN): cpc2_hip.h,
    cpc_async_error_check.  Called where the loop synchronises with the device anyway."""
    from . import _lib
    _lib.check(_lib.load().cpc_async_error_check(_lib.stream_ptr(torch.device(device))), "async error check")


def trainStep(dataLoader, cpcModel, cpcCriterion, optimizer, scheduler, loggingStep, dp=None, device=None):
    """train.py:72-142.  `dataLoader` yields (sequence [b,2,1,L], label [b][, signal_quality])."""
    cpcModel.train()
    cpcCriterion.train()
    device = device or next(cpcModel.parameters()).device
    dp = dp or DataParallelContext.for_modules(optimizer, cpcModel, cpcCriterion)      # (run() builds it once and passes it)
    start_time = time.perf_counter()
    n_examples, it = 0, 0
    sum_loss = sum_acc = None
    logs = {}
    for step, full_data in enumerate(dataLoader):
        sequence, label, *signal_quality = full_data
        sequence = sequence.to(device, non_blocking=True)
        label = label.to(device, non_blocking=True)
        signal_quality = signal_quality[0].to(device, non_blocking=True) if len(signal_quality) else None
        past, future = sequence[:, 0, ...], sequence[:, 1, ...]
        n_examples += past.size(0)
        totLoss, allLosses, allAcc = cpcStep(past, future, label, cpcModel, cpcCriterion, signal_quality, dp=dp)
        backward(totLoss)
        dp.reduce_and_step()
        optimizer.zero_grad()
        if allLosses.nelement() > 0:
            it += 1
            ls, ac = allLosses.detach().mean(dim=0), allAcc.mean(dim=0)
            sum_loss = ls if sum_loss is None else sum_loss + ls
            sum_acc = ac if sum_acc is None else sum_acc + ac
            if (step + 1) % loggingStep == 0:
                elapsed = time.perf_counter() - start_time
                print(f"Update {step + 1}\nelapsed: {elapsed:.1f} s")
                print(f"{1000.0 * elapsed / loggingStep:.1f} ms per batch, {1000.0 * elapsed / n_examples:.1f} ms / example")
                print("locLoss_train", (sum_loss / it).cpu().numpy())
                _check_async(device)                      # the copy above synchronised anyway
                start_time, n_examples = time.perf_counter(), 0
    if scheduler is not None:
        scheduler.step()
    _check_async(device)
    if it > 0:
        logs["locLoss_train"] = (sum_loss / it).cpu().numpy()
        logs["locAcc_train"] = (sum_acc / it).cpu().numpy()
    logs["iter"] = it
    return logs


def valStep(dataLoader, cpcModel, cpcCriterion, device=None):
    """train.py:145-187."""
    cpcCriterion.eval()
    cpcModel.eval()
    device = device or next(cpcModel.parameters()).device
    it = 0
    sum_loss = sum_acc = None
    for full_data in dataLoader:
        sequence, label, *_ = full_data
        sequence, label = sequence.to(device, non_blocking=True), label.to(device, non_blocking=True)
        past, future = sequence[:, 0, ...], sequence[:, 1, ...]
        with torch.no_grad():
            _, allLosses, allAcc = cpcStep(past, future, label, cpcModel, cpcCriterion, None)
        it += 1
        ls, ac = allLosses.mean(dim=0), allAcc.mean(dim=0)
        sum_loss = ls if sum_loss is None else sum_loss + ls
        sum_acc = ac if sum_acc is None else sum_acc + ac
    logs = {"iter": it}
    _check_async(device)
    if it > 0:
        logs["locLoss_val"] = (sum_loss / it).cpu().numpy()
        logs["locAcc_val"] = (sum_acc / it).cpu().numpy()
    return logs


def run(trainDataset, valDataset, batchSize, samplingMode, cpcModel, cpcCriterion, nEpoch, pathCheckpoint, optimizer,
        scheduler, logs, no_artefacts=False, batchSizePerGPU=None, dp=None, is_master=True):
    """The epoch loop of train.py:190-255: per epoch a fresh train loader (random offsets) and a sequential
    validation loader, trainStep, valStep, the logs dict extended key by key, and every logs["saveStep"] epochs (and
    after the last one) a checkpoint `{pathCheckpoint}_{epoch}.pt` in the reference layout plus `_logs.json`.
    Resumes from len(logs["epoch"]).  Like the reference, `best` holds the model state of the last epoch whose
    validation accuracy beat bestAcc -- which is never raised from 0 (train.py:207,237-238)."""
    import json
    from . import feature_loader as fl
    # built ONCE (its constructor broadcasts rank 0's parameters): the criterion's and the context network's gradient
    # slices are reduced under the encoder's backward, as bench.py measures it
    dp = dp or DataParallelContext.for_modules(optimizer, cpcModel, cpcCriterion)
    print(f"Running {nEpoch} epochs")
    best_acc, best_state = 0, None
    t_start = time.perf_counter()
    # Everything alive by now (modules, optimiser state, the dataset's buffers) lives as long as the run: moved out of the cyclic
    # collector's way, so that its occasional full pass does not stop the training thread for longer than its lead over the device
    # (70-165 ms about once per 15-25 thousand steps with torch's objects in the walk: profiles/r06_long_soak.txt).  Objects made
    # from here on are collected as before.
    import gc
    gc.collect()
    gc.freeze()
    for epoch in range(len(logs["epoch"]), nEpoch):
        print(f"Starting epoch {epoch}")
        train_loader = trainDataset.getDataLoader(batchSize, samplingMode, True, numWorkers=0, remove_artefacts=no_artefacts,
                                                  batch_size_per_gpu=batchSizePerGPU)
        val_loader = valDataset.getDataLoader(batchSize, "sequential", False, numWorkers=0)
        print("Training dataset %d batches, Validation dataset %d batches, batch size %d"
              % (len(train_loader), len(val_loader), batchSize))
        epoch_logs = trainStep(train_loader, cpcModel, cpcCriterion, optimizer, scheduler, logs["logging_step"], dp=dp)
        epoch_logs.update(valStep(val_loader, cpcModel, cpcCriterion))
        print(f"Ran {epoch + 1} epochs in {time.perf_counter() - t_start:.2f} seconds")
        if "locAcc_val" in epoch_logs and float(epoch_logs["locAcc_val"].mean()) > best_acc:
            best_state = {k: v.detach().clone() for k, v in fl.get_module(cpcModel).state_dict().items()}
        for key, value in epoch_logs.items():
            logs.setdefault(key, [None] * epoch).append(value.tolist() if isinstance(value, np.ndarray) else value)
        logs["epoch"].append(epoch)
        if pathCheckpoint is not None and is_master and (epoch % logs["saveStep"] == 0 or epoch == nEpoch - 1):
            fl.save_checkpoint(fl.get_module(cpcModel).state_dict(), fl.get_module(cpcCriterion).state_dict(),
                               optimizer.state_dict(), best_state, f"{pathCheckpoint}_{epoch}.pt")
            with open(pathCheckpoint + "_logs.json", "w") as fh:
                json.dump(logs, fh, indent=2)
    return logs


def init_distributed_mode(backend="nccl"):
    """distributed_mode.py:75-142 reduced to the torch.distributed.run environment: RANK, LOCAL_RANK,
    WORLD_SIZE, MASTER_ADDR/PORT; one process per GPU; backend 'nccl' is RCCL on ROCm."""
    import os
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if backend == "nccl":
        torch.cuda.set_device(local_rank)
    if world > 1 and not dist.is_initialized():
        dist.init_process_group(init_method="env://", backend=backend, world_size=world, rank=rank)
    return rank, local_rank, world


# --------------------------------------------------------------------------- the command line (train.py:260-688)
def set_seed(seed):
    """cpc/utils/misc.py:63-68: python's, torch's (host and every device) and numpy's generators."""
    import random
    random.seed(seed)
    torch.manual_seed(seed)
    np.random.seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def splitTrainVal(seqTrain, samplingType):
    """train.py:322-341: shuffle (python's generator), then the first 95 % train and the rest validate.  Under
    temporalsamespeaker the shuffle moves whole runs of equal speaker index, so that a speaker's files keep their order."""
    import itertools
    import random
    if samplingType == "temporalsamespeaker":
        blocks = [list(run) for _spk, run in itertools.groupby(seqTrain, key=lambda item: item[0])]
        random.shuffle(blocks)
        seqTrain = list(itertools.chain.from_iterable(blocks))
    else:
        seqTrain = list(seqTrain)
        random.shuffle(seqTrain)
    sizeTrain = int(0.95 * len(seqTrain))
    return seqTrain[:sizeTrain], seqTrain[sizeTrain:]


def loadCriterion(pathCheckpoint, downsampling, nSpeakers, nPhones=None):
    """train.py:62-69: the criterion of the run that wrote pathCheckpoint (built from ITS arguments), weights loaded."""
    import os
    from . import feature_loader as fl
    _, _, locArgs = fl.getCheckpointData(os.path.dirname(pathCheckpoint))
    criterion = getCriterion(locArgs, downsampling, nSpeakers, nPhones)
    criterion.load_state_dict(torch.load(pathCheckpoint, 'cpu')["cpcCriterion"])
    return criterion


TEMPORAL_CONVENTIONS = ['id_spkr_onset_offset', 'id_spkr_onset_offset_spkr_onset_offset', 'spkr-id', 'spkr_id_nb',
                        'spkr-id-nb', 'no_speaker', 'full_seedlings']
# train.py:273-277: what a resumed run takes from ITS command line, not from the checkpoint's arguments
FORBIDDEN_ON_RESUME = {"nGPU", "pathCheckpoint", "debug", "restart", "world_size", "global_rank", "local_rank", "n_nodes",
                       "node_id", "n_gpu_per_node", "max_size_loaded", "nEpoch", "save_step"}


def parseArgs(argv):
    """train.py:550-682: the same groups, flags, defaults, derived values and errors."""
    import argparse
    import os
    import random
    import sys
    from .cpc_default_config import set_default_cpc_config
    parser = set_default_cpc_config(argparse.ArgumentParser(description='Trainer', prog='python -m cpc2_amd.train'))
    g = parser.add_argument_group('Dataset')
    g.add_argument('--pathDB', type=str, default=None, help='Directory of the audio files.')
    g.add_argument('--file_extension', type=str, default=".flac", help='Extension of the audio files.')
    g.add_argument('--pathTrain', type=str, default=None, help='Text file listing the training sequences.')
    g.add_argument('--pathVal', type=str, default=None, help='Text file listing the validation sequences.')
    g.add_argument('--n_process_loader', type=int, default=8, help='Accepted; files are decoded in this process.')
    g.add_argument('--ignore_cache', action='store_true',
                   help='List the data set again instead of reading its sequence cache (which is keyed by nothing: use '
                        'this after changing the data, the extension, --naming_convention or --no_speaker).')
    g.add_argument('--path_cache', type=str, default=None,
                   help='Where the sequence cache lives (default: _seqs_cache.txt inside --pathDB).')
    g.add_argument('--max_size_loaded', type=int, default=4000000000, help='Samples resident on the device at a time.')
    g = parser.add_argument_group('Supervised mode (refused: see cpc2_amd.eval.linear_separability --unfrozen)')
    g.add_argument('--supervised', action='store_true')
    g.add_argument('--pathPhone', type=str, default=None)
    g.add_argument('--CTC', action='store_true')
    g = parser.add_argument_group('Save')
    g.add_argument('--pathCheckpoint', type=str, default=None, help='Output directory.')
    g.add_argument('--logging_step', type=int, default=1000)
    g.add_argument('--save_step', type=int, default=5, help='Epochs between two checkpoints.')
    g = parser.add_argument_group('Load')
    g.add_argument('--load', type=str, default=None, nargs='*',
                   help='A checkpoint (.pt) to start from; its directory holds checkpoint_args.json and checkpoint_logs.json.')
    g.add_argument('--loadCriterion', action='store_true', help='With --load: the criterion weights too.')
    g.add_argument('--restart', action='store_true', help='Ignore the checkpoints found in --pathCheckpoint.')
    g = parser.add_argument_group('GPUs')
    g.add_argument('--nGPU', type=int, default=-1,
                   help='One GPU per process here: 1 (or 0); -1 resolves to the device count. Several GPUs: --distributed.')
    g.add_argument('--batchSizeGPU', type=int, default=8, help='Windows per batch and GPU.')
    parser.add_argument('--debug', action='store_true', help='Keep the last 1000 / 100 files only.')
    g = parser.add_argument_group('Distributed training')
    g.add_argument('--distributed', action='store_true', help='One process per GPU, started by torch.distributed.run.')
    g.add_argument("--local_rank", type=int, default=-1)
    g.add_argument("--master_port", type=int, default=-1)
    args = parser.parse_args(argv)

    if args.pathDB is None and (args.pathCheckpoint is None or args.restart):
        parser.print_help()
        print("Either provides an input dataset or a checkpoint to load")
        sys.exit()
    assert args.bandreject_scaler >= 0
    if args.samplingType == "temporalsamespeaker" and (args.pathTrain is not None or args.pathVal is not None):
        raise ValueError("Can not apply temporal sampling (with same speaker) if pathTrain or pathVal is specified.\n"
                         "Sequences are loaded in temporal order, and a list of utterances could break it.")
    if args.samplingType == "temporalsamespeaker" and args.naming_convention not in TEMPORAL_CONVENTIONS:
        raise ValueError("temporalsamespeaker sampling needs --naming_convention (one of %s): the files have to be sorted in "
                         "time." % TEMPORAL_CONVENTIONS)
    if not args.meta_aug and (args.meta_aug_type is not None or args.meta_aug_type == "none"):
        raise ValueError("You specified parameters --meta_aug_type without having activated --meta_aug flag.")
    if args.meta_aug and args.meta_aug_type is None or args.meta_aug_type == "none":
        raise ValueError("You specified flag --meta_aug, but you haven't specified meta_aug_type")
    if args.pathCheckpoint is not None:
        args.pathCheckpoint = os.path.abspath(args.pathCheckpoint)
    if args.load is not None:
        args.load = [os.path.abspath(x) for x in args.load]
    if args.random_seed is None:                        # drawn here so that it is dumped with the other arguments
        args.random_seed = random.randint(0, 2**31)
    if args.nGPU < 0:
        args.nGPU = torch.cuda.device_count()
    assert args.nGPU <= torch.cuda.device_count(), \
        f"number of GPU asked: {args.nGPU}, number GPU detected: {torch.cuda.device_count()}"
    print(f"Let's use {args.nGPU} GPUs!")
    if args.arMode == 'no_ar':
        args.hiddenGar = args.hiddenEncoder
    return args


def refuseUnsupported(args):
    """What the command line accepts (for the sake of checkpoint_args.json) and this package does not do: refused with the
    flag's name and, where there is one, the way that works -- before any file is read."""
    if args.nGPU > 1 and not args.distributed:
        raise SystemExit(f"--nGPU {args.nGPU}: this package runs one GPU per process (there is no DataParallel wrapper); run "
                         f"with --nGPU 1, or one process per GPU: python -m torch.distributed.run --nproc_per_node {args.nGPU} "
                         "-m cpc2_amd.train --distributed ...")
    from .data_augmentation import BUILT_TYPES, FILTER_TYPES, OWN_TYPES, unbuilt_message
    asked = list(args.augment_type) if args.augment_type is not None else []
    if (args.augment_past or args.augment_future) and any(t not in BUILT_TYPES + OWN_TYPES + FILTER_TYPES and t != 'none' for t in asked):
        raise NotImplementedError(unbuilt_message(asked))
    if args.encoder_type in ("mfcc", "lfb"):
        raise NotImplementedError(f"--encoder_type {args.encoder_type}: only the raw-waveform encoder (--encoder_type cpc) is built")
    if args.cpc_mode == "bert":
        raise NotImplementedError("--cpc_mode bert: the BERT objective is not built (--cpc_mode reverse, none, or no flag)")
    if args.normMode != "layerNorm":
        raise NotImplementedError(f"--normMode {args.normMode}: the encoder kernels normalise with layerNorm only")
    if args.rnnMode in ("ffd", "conv4", "conv8", "conv12", "transformer_adaptive_span"):
        raise NotImplementedError(f"--rnnMode {args.rnnMode}: the predictors with a kernel path are linear, transformer, LSTM "
                                  "and RNN")
    if args.multihead_rnn and args.rnnMode != "transformer":
        raise NotImplementedError(f"--multihead_rnn with --rnnMode {args.rnnMode}: the multi-head predictor is a transformer "
                                  "(--rnnMode transformer)")
    if args.supervised:
        raise NotImplementedError("--supervised: the supervised criteria are not trained through this loop (in the reference this "
                                  "path fails at the first step: its trainStep hands the criterion an argument too many); train "
                                  "them with python -m cpc2_amd.eval.linear_separability --unfrozen")


def main(argv):
    """cpc/train.py:260-547, step for step: a checkpoint found in --pathCheckpoint is resumed (its arguments win except
    FORBIDDEN_ON_RESUME), the seed, the CONFIG dump, the listing (findAllSeqs with the naming convention and the sequence
    cache), --pathTrain / --pathVal or the 95 / 5 split, --debug, the per-rank shard, the two AudioBatchData, the model and
    criterion (--load [--loadCriterion], or built from the arguments), the optimiser (state loaded on resume),
    checkpoint_args.json, the scheduler fast-forwarded over the epochs done, run().  Returns a namespace of what it built
    (args, logs, cpcModel, cpcCriterion, optimizer, scheduler).

    Where this package departs from the reference, so does main:
      * no DataParallel / DistributedDataParallel wrappers: run() builds a DataParallelContext.  One GPU per process --
        --nGPU above 1 without --distributed is refused; --distributed reads the torch.distributed.run environment
        (init_distributed_mode) instead of SLURM's;
      * what refuseUnsupported lists is refused before any file is read (and again for the arguments of a resumed run);
      * augmentation (train.py:356-419): the noise data set's keep_temporality follows the reference's test on
        --naming_convention, and no convention counts as False (the reference crashes on None there); under --distributed
        every rank uses the whole noise set (the reference shards the list after the data set is built, which changes nothing);
        `additive` without --pathDBNoise raises before the speech data is loaded; validation data is never augmented;
      * no validation sequence is an error here (the reference builds no validation set and fails inside run());
      * logs that lack saveStep / logging_step (a hand-made run directory) get them from the command line;
      * audio files are decoded in this process: --n_process_loader is accepted and unused."""
    import os
    from . import feature_loader as fl
    from .data_augmentation import augmentation_factory
    from .dataset import AudioBatchData, PeakNorm, filterSeqs, findAllSeqs, shard_for_rank
    args = parseArgs(argv)
    refuseUnsupported(args)

    logs = {"epoch": [], "iter": [], "saveStep": args.save_step}
    logs["logging_step"] = args.logging_step
    loadOptimizer = False
    if args.pathCheckpoint is not None and not args.restart:
        cdata = fl.getCheckpointData(args.pathCheckpoint)
        if cdata is not None:
            data, logs, locArgs = cdata
            print(f"Checkpoint detected at {data}")
            fl.loadArgs(args, locArgs, forbiddenAttr=FORBIDDEN_ON_RESUME)
            args.load, loadOptimizer = [data], True
            args.loadCriterion = True
            refuseUnsupported(args)
            logs.setdefault("saveStep", args.save_step)         # (a hand-made run directory: run() reads both)
            if args.random_seed is None:                        # (... whose arguments may hold no seed either)
                import random
                args.random_seed = random.randint(0, 2**31)
    logs["logging_step"] = args.logging_step
    if args.nGPU == 0:
        args.nGPU = 1
    if args.pathDB is None:
        raise ValueError("--pathDB is missing and the checkpoint's arguments hold none")
    if args.signal_quality_path is not None and not os.path.exists(args.signal_quality_path):
        raise ValueError("%s can't be found. Are you sure you provided the right location ?" % args.signal_quality_path)
    batchSize = args.nGPU * args.batchSizeGPU

    if args.distributed:
        print('Distributed mode, moving to 1 process for data loading')
        args.n_process_loader = 1
        args.global_rank, args.local_rank, args.world_size = init_distributed_mode()
    args.is_local_master = (not args.distributed) or (args.global_rank == 0)

    set_seed(args.random_seed)
    print(f'CONFIG:\n{json.dumps(vars(args), indent=4, sort_keys=True)}')
    print('-' * 50)

    seqNames, speakers = findAllSeqs(args.pathDB, no_speaker=args.no_speaker, extension=args.file_extension,
                                     loadCache=not args.ignore_cache, format=args.naming_convention,
                                     cache_path=args.path_cache)
    print(f'Found files: {len(seqNames)} seqs, {len(speakers)} speakers')
    seqTrain = filterSeqs(args.pathTrain, seqNames) if args.pathTrain is not None else seqNames
    if len(seqTrain) == 0:
        raise ValueError("No training sequences can be found. Please check that you provided the right path, and specified "
                         "the right audio extension.")
    if args.pathVal is None:
        print('No validation data specified!')
        seqTrain, seqVal = splitTrainVal(seqTrain, args.samplingType)
        print(f'Found files: {len(seqTrain)} train, {len(seqVal)} val')
    else:
        seqVal = filterSeqs(args.pathVal, seqNames)
    if args.debug:
        seqTrain = seqTrain[-1000:]
        seqVal = seqVal[-100:]
    if args.distributed:
        print(f'Initial worker files: {len(seqTrain)} train, {len(seqVal)} val')
        seqTrain = shard_for_rank(seqTrain, args.global_rank, args.world_size)
        seqVal = shard_for_rank(seqVal, args.global_rank, args.world_size)
        print(f'Current worker files: {len(seqTrain)} train, {len(seqVal)} val')
    if not seqTrain:
        raise ValueError("No training sequences are left after the train / validation split (a single file goes to validation).")
    if not seqVal:
        raise ValueError("No validation sequences: the 95 / 5 split (or --pathVal) left none, and every epoch validates. "
                         "Give more files, or --pathVal.")

    # train.py:356-385: the noise data set (one speaker, PeakNorm, its own augmentation under --meta_aug)
    noiseDataset = None
    augmenting = args.augment_past or args.augment_future
    if augmenting and args.augment_type and 'additive' in args.augment_type and args.pathDBNoise is None:
        raise RuntimeError('Noise dataset is needed for the additive noise')
    if args.pathDBNoise is not None and augmenting:
        seqNoise, _ = findAllSeqs(args.pathDBNoise, extension=args.noise_extension, loadCache=True, speaker_level=0)
        if args.pathSeqNoise is not None:
            seqNoise = filterSeqs(args.pathSeqNoise, seqNoise)
        if args.debug:
            seqNoise = seqNoise[:100]
        print(f'\nLoading noise data at {args.pathDBNoise}')
        print("Loading the noise dataset")
        noiseDataset = AudioBatchData(args.pathDBNoise, args.sizeWindow, seqNoise, None, 1, transform=PeakNorm(),
                                      nProcessLoader=args.n_process_loader, MAX_SIZE_LOADED=args.max_size_loaded,
                                      augment_future=False, augment_past=args.meta_aug,
                                      augmentation=augmentation_factory(args, noiseDataset, applied_on_noise=True),
                                      keep_temporality=(args.naming_convention or "").startswith("id_spkr_onset_offset"),
                                      past_equal_future=args.meta_aug)

    print(f'\nLoading audio data at {args.pathDB}')
    print("Loading the training dataset")
    augmentation = augmentation_factory(args, noiseDataset)      # (before the audio is read: its errors come first)
    trainDataset = AudioBatchData(args.pathDB, args.sizeWindow, seqTrain, None, len(speakers),
                                  nProcessLoader=args.n_process_loader, MAX_SIZE_LOADED=args.max_size_loaded,
                                  augment_future=args.augment_future, augment_past=args.augment_past,
                                  augmentation=augmentation,
                                  keep_temporality=args.samplingType == "temporalsamespeaker",
                                  signal_quality_path=args.signal_quality_path, signal_quality_step=args.signal_quality_step,
                                  signal_quality_mode=args.signal_quality_mode, past_equal_future=args.past_equal_future)
    print("Training dataset loaded\n")
    print("Loading the validation dataset")
    valDataset = AudioBatchData(args.pathDB, args.sizeWindow, seqVal, None, len(speakers),
                                nProcessLoader=args.n_process_loader)
    print("Validation dataset loaded\n")
    device = torch.device("cuda", torch.cuda.current_device())       # (the feeder's default device too)

    if args.load is not None:
        cpcModel, args.hiddenGar, args.hiddenEncoder = fl.loadModel(args.load)
    else:
        cpcModel = CPCModel(getEncoder(args), getAR(args), args.mask_prob, args.mask_length)
    downsampling = cpcModel.gEncoder.DOWNSAMPLING
    print(args)
    if args.load is not None and args.loadCriterion:
        cpcCriterion = loadCriterion(args.load[0], downsampling, len(speakers), None)
    else:
        cpcCriterion = getCriterion(args, downsampling, len(speakers), None)
    if loadOptimizer:
        cpcCriterion.load_state_dict(torch.load(args.load[0], 'cpu')["cpcCriterion"])
    cpcCriterion.to(device)
    cpcModel.to(device)

    print("Using Adam optimizer." if args.optimizer == 'adam' else "Using SGD optimizer.")
    optimizer = buildOptimizer(cpcModel, cpcCriterion, lr=args.learningRate, beta1=args.beta1, beta2=args.beta2,
                               epsilon=args.epsilon, optimizer=args.optimizer)
    if loadOptimizer:
        print("Loading optimizer " + args.load[0])
        state_dict = torch.load(args.load[0], 'cpu')
        if "optimizer" in state_dict:
            optimizer.load_state_dict(state_dict["optimizer"])

    if args.pathCheckpoint is not None:
        os.makedirs(args.pathCheckpoint, exist_ok=True)
        args.pathCheckpoint = os.path.join(args.pathCheckpoint, "checkpoint")
        if args.is_local_master:
            with open(args.pathCheckpoint + "_args.json", 'w') as file:
                json.dump(vars(args), file, indent=2)

    if args.schedulerRamp is not None:
        print(f"Ramp activated. n_e = {args.schedulerRamp}")
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                 # (fast-forwarding steps the scheduler before the optimiser, as the reference does)
        scheduler = buildScheduler(optimizer, args.schedulerStep, args.schedulerRamp, epochs_done=len(logs["epoch"]))

    print('args.local_rank: ' + str(args.local_rank))
    run(trainDataset, valDataset, batchSize, args.samplingType, cpcModel, cpcCriterion, args.nEpoch,
        args.pathCheckpoint if args.is_local_master else None, optimizer, scheduler, logs, args.no_artefacts,
        args.batchSizeGPU)
    import types
    return types.SimpleNamespace(args=args, logs=logs, cpcModel=cpcModel, cpcCriterion=cpcCriterion, optimizer=optimizer,
                                 scheduler=scheduler)


if __name__ == "__main__":
    import sys
    from cpc2_amd.train import main as _main        # (the package's copy of this module, not the __main__ one)
    _main(sys.argv[1:])
