"""cpc_encoder_forward / cpc_encoder_backward over the domain include/cpc2_hip.h states: the forward from 159 samples on, the backward
from 400 samples on, any window count, hidden 32 .. 512, one or two input batches (x_rest), deferred 0 / 1 -- and what they refuse.

Reference: oracle.cpc_oracle.encoder_forward in fp64, differentiated by autograd; parameters from oracle.synth.encoder_params,
windows from synth.audio_windows, the upstream gradient dz from synth.features.  Every oracle run collects the five layers'
pre-activations and asserts that none lies within RELU_MARGIN of zero relative to its layer's largest (oracle/settle.py: a ReLU
decision inside fp32 rounding says nothing about the arithmetic under test).  That assertion guards the INPUTS, it is no tolerance on
the kernels.  Each case records its seed (Case.seed = 131 hidden + 17 n + length: parameters 7000 + seed, windows 7100 + seed, dz
7200 + seed).  A seed alone settles only the smallest cases -- about 3 in 1e5 pre-activations lie inside the margin, and these cases
have 4e3 .. 3e6 of them -- so settle.settle_encoder_relu_decisions then raises batchNorm{i}.bias of the channels concerned by 3
margins, judged by the fp64 numbers alone, in the fp32 parameters both sides load.  No element is excluded from any comparison.

Harness.  Every buffer of a call -- x_first, x_rest, the 20 parameters, dz, z, the 20 gradients, saved, scratch -- is a window of a
larger allocation filled with ONE quiet-NaN bit pattern (NAN_WORD) and guarded on both sides; z, the gradients, saved and scratch hold
the pattern when the forward starts, scratch is filled again between forward and backward; saved and scratch are exactly
cpc_encoder_saved_bytes / _scratch_bytes long.  After each of the two calls every word outside the windows must be unchanged and
every input bit for bit; afterwards every element of z and of each gradient is finite and within the project's tolerances for the
encoder at few windows (tests/test_gpu_parity.py::test_encoder_vs_oracle_fp64: z 2e-5, gradients 2e-4 of the reference's largest
element, and element by element atol + 64 tol |ref|).  So the library stays inside the sizes it reports, reads no row of saved or
scratch it did not write (the halo and slack rows of the products: a NaN would reach an output as 0 * NaN), keeps nothing in scratch
between the passes and overwrites the gradients.  With deferred = 1 the gradients are read after cpc_side_tail_join.  Every case ends
with cpc_async_error_check.  Nothing relies on a fault.

Families (the unmarked tests at the end hold the list to this with a Python restatement of enc_layout's L[i], `even`, the
weight-gradient product's rows R and the f32 path's rounds_seg < rounds_full):
  A  all 16 patterns of the per-layer `even` branch (L[i] == s L[i+1], layers 1..4), 400 .. 547 samples, at hidden 256 and 512 with
     n such that n (frames + 2) >= 64, and at hidden 64 with n = 3
  B  the weight-gradient product's R = n (frames + 2) on both sides of 64 at hidden 256 / 512 (one window has 64 rows from 9919
     samples on, not 9920: 9918 samples are there for the 63).  R < 64 RUNS: the host driver pads
     the reduction with zero rows of dU (tn_rows, cpc2_amd/csrc/encoder.hip; no kernel changed) -- the first of the two ways the
     issue allowed, so these cases compare numbers like all others and nothing is refused from 400 samples on
  C  every hidden size at n = 1: 400, 479, 547, 2560, 3300 samples
  D  x_rest: n_first = 1 and n - 1 of n = 3, bit-identical to the one-buffer call
  E  deferred 0 against 1, gradients bit-identical after the join
  F  refusals: nothing launched, the poison intact in every window, the library works afterwards

Worst relative errors per family, measured on an MI355X (python -m pytest tests/test_encoder_abi_gpu.py -m gpu -s prints the table
per case), against z 2e-5 / grad 2e-4:
  family                                              z          grad       worst case (z / grad)
  A  the 16 `even` patterns, hidden 256 / 512 / 64    9.3e-07    2.3e-06    h64 n3 539 samples / h512 n16 400 samples
  B  R = n (frames + 2) around 64, hidden 256 / 512   8.9e-07    2.4e-06    h256 n1 20480 samples / h512 n2 4800 samples
  C  every hidden size, one window                    1.1e-06    1.6e-06    h128 2560 samples / h512 3300 samples
  D  x_rest (both splits give the same figures)       9.0e-07    1.3e-06    h128 539 samples / h256 404 samples
  E  deferred (the same figures as deferred = 0)      8.3e-07    2.4e-06    h256 n16 404 samples / h512 n2 4800 samples
The f32-torch evaluation of the oracle is off by 2.2e-07 .. 6.7e-07 (z) and 4.9e-07 .. 2.5e-06 (gradients) on the same cases
(on one host thread: with 8 threads torch's f32 conv backward returned gradients off by 0.1 .. 0.4 on five cases at hidden 512, 13 /
16 windows, where one thread gives 1.4e-06 and the fp64 run is unaffected -- the host tests below evaluate on one thread).
The cases of B below 64 rows, which the backward refused before the driver padded them (z / worst gradient): h256 n1 400 samples
4.2e-07 / 1.0e-06, n15 7.6e-07 / 1.3e-06, n1 4800 samples 5.7e-07 / 1.1e-06, n1 9918 samples 6.6e-07 / 1.4e-06; h512 n1 400 samples
3.9e-07 / 1.3e-06, n15 6.4e-07 / 2.1e-06, n1 4800 samples 5.3e-07 / 1.5e-06, n1 9918 samples 6.5e-07 / 2.0e-06 (and all of C at 256 / 512).
The project tolerances hold on every case, so no family has a bound of its own (it would have been 4 x the error of the f32-torch
evaluation of the oracle on the same case, never a figure taken from the kernels).
"""
import collections
import functools
import math

import pytest
import torch

from cpc2_amd import _lib
from oracle import cpc_oracle as O
from oracle import synth
from oracle.settle import RELU_MARGIN, settle_encoder_relu_decisions

DEV = "cuda:0"
NAN_WORD = 0x7FC0BEEF              # the one bit pattern of every poisoned word: a quiet NaN no arithmetic produces
GUARD = 64                         # words of poison before and behind every window
EPS = 1e-5
TOL_Z, TOL_GRAD = 2e-5, 2e-4       # tests/test_gpu_parity.py::test_encoder_vs_oracle_fp64 (few windows)
PREFIX = "gEncoder."
GEOMETRY = O.ENCODER_GEOMETRY      # (kernel, stride, padding) of the five convolutions

_WORST = {}         # case id -> {"z" | "grad": (worst relative error, where)}


# ------------------------------------------------------------------------------------------- enc_layout, restated (no GPU, no library)
def frames_after(length):
    """L[0..5]: samples, then frames after layers 0..4 (0 from the first layer on that leaves none)."""
    L = [length]
    for k, s, p in GEOMETRY:
        span = L[-1] + 2 * p - k
        L.append(span // s + 1 if span >= 0 and L[-1] > 0 else 0)
    return L


def even_pattern(length):
    """'1' where the backward-data product of layer 1..4 takes the whole-tiles + boundary-row branch: L[i] == s L[i+1]."""
    L = frames_after(length)
    return "".join("1" if L[i] == GEOMETRY[i][1] * L[i + 1] else "0" for i in range(1, 5))


def tn_rows(n, length, layer=4):
    """Reduction rows of layer `layer`'s weight-gradient product: n (L_out + 2); layer 4's are the fewest."""
    return n * (frames_after(length)[layer + 1] + 2)


def two_product_layers(hidden, n, length):
    """Layers of the f32 path (hidden < 256) whose backward-data runs as a main product over seg_valid rows + a boundary product."""
    if hidden % 256 == 0:
        return []
    L, hit = frames_after(length), []
    for i in range(1, 5):
        s = GEOMETRY[i][1]
        col_blocks = max(1, s * hidden // 256)
        rounds_full = -(-(-(-n * (L[i + 1] + 2) // 128) * col_blocks) // 512)
        rounds_seg = -(-(n * -(-L[i + 1] // 128) * col_blocks) // 512)
        if L[i] == s * L[i + 1] and rounds_seg < rounds_full:
            hit.append(i)
    return hit


# ----------------------------------------------------------------------------------------------------------------- the cases
# hidden, n windows of `length` samples; n_first: 0 = one input batch, else windows n_first .. n - 1 come from x_rest
Case = collections.namedtuple("Case", "family hidden n length n_first deferred seed")


def _case(family, hidden, n, length, n_first=0, deferred=0):
    return Case(family, hidden, n, length, n_first, deferred, 131 * hidden + 17 * n + length)


def _id(c):
    parts = [c.family, f"h{c.hidden}", f"n{c.n}", f"len{c.length}"]
    parts += [f"first{c.n_first}"] if c.n_first else []
    parts += ["deferred"] if c.deferred else []
    return "-".join(parts)


# samples -> the pattern of `even` over layers 1..4 (all 16 occur between 400 and 547 samples)
EVEN_LENGTHS = {464: "0000", 544: "0001", 424: "0010", 504: "0011", 444: "0100", 524: "0101", 404: "0110", 484: "0111",
                459: "1000", 539: "1001", 419: "1010", 499: "1011", 439: "1100", 519: "1101", 400: "1110", 479: "1111"}


def _n_for_64_rows(length):
    return -(-64 // (frames_after(length)[5] + 2))            # 16 at two frames, 13 at three


CASES_A = ([_case("A", hidden, _n_for_64_rows(length), length) for hidden in (256, 512) for length in EVEN_LENGTHS]
           + [_case("A", 64, 3, length) for length in EVEN_LENGTHS])
CASES_B = [_case("B", hidden, n, length) for hidden in (256, 512)
           for n, length in ((1, 400), (15, 400), (16, 400), (1, 4800), (2, 4800), (1, 9918), (1, 9919), (1, 9920), (1, 20480))]
CASES_C = [_case("C", hidden, 1, length) for hidden in (32, 64, 128, 256, 512) for length in (400, 479, 547, 3300, 2560)]
CASES_D = [_case("D", hidden, 3, length, n_first=n_first) for hidden in (256, 128) for length in (404, 539) for n_first in (1, 2)]
_SHAPES_E = [(256, 16, 464), (256, 16, 404), (512, 13, 479), (512, 13, 539), (512, 2, 4800)]
CASES_E = [_case("E", hidden, n, length, deferred=1) for hidden, n, length in _SHAPES_E]
CASES = CASES_A + CASES_B + CASES_C


# ------------------------------------------------------------------------------------------------------ values and references
Problem = collections.namedtuple("Problem", "p x dz z grads raised")
NAMES = [f"{PREFIX}{kind}{i}.{leaf}" for i in range(5) for kind, leaf in (("conv", "weight"), ("conv", "bias"), ("batchNorm", "weight"),
                                                                          ("batchNorm", "bias"))]      # the C ABI's order


def oracle_forward(x, p, check_margin=True, forward_fn=None):
    """z [n, frames, H] channel-last, in the dtype of x and p."""
    if forward_fn is not None:
        return forward_fn(x, p).permute(0, 2, 1)
    pre = []
    out = O.encoder_forward(x, p, PREFIX, pre_out=pre)
    if check_margin:
        for i, y in enumerate(pre):
            floor = float(y.abs().min() / y.abs().max())
            assert floor >= RELU_MARGIN, f"layer {i}: a ReLU decision within {RELU_MARGIN} of zero (relative {floor:.2e})"
    return out.permute(0, 2, 1)


def differentiate(x, p, dz, dtype, **kw):
    """(z, {name: gradient}) of sum(z * dz) with everything held in `dtype`."""
    pd = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in p.items()}
    z = oracle_forward(x.to(dtype), pd, **kw)
    (z * dz.to(dtype)).sum().backward()
    return z.detach(), {k: v.grad for k, v in pd.items()}


def _shape_key(c):
    """The fields the values and the reference depend on (not: the argument forms)."""
    return c._replace(family="", n_first=0, deferred=0)


@functools.lru_cache(maxsize=2)
def _problem(key):
    c = key
    p = synth.encoder_params(c.hidden, 7000 + c.seed, prefix=PREFIX)
    assert list(p) == NAMES
    x = synth.audio_windows(c.n, c.length, 7100 + c.seed)
    dz = synth.features((c.n, frames_after(c.length)[5], c.hidden), 7200 + c.seed)
    raised = settle_encoder_relu_decisions(p, PREFIX, x)
    return Problem(p, x, dz, *differentiate(x, p, dz, torch.float64), raised)


def problem_of(c):
    return _problem(_shape_key(c))


# ------------------------------------------------------------------------------------------------------------------ buffers
class Guarded:
    """An allocation of GUARD + words + GUARD int32 words, all NAN_WORD; .f32 is the window as floats."""

    def __init__(self, words, device):
        self.words = int(words)
        self.all = torch.full((2 * GUARD + self.words,), NAN_WORD, dtype=torch.int32, device=device)
        self.f32 = self.all[GUARD:GUARD + self.words].view(torch.float32)

    def poison(self):
        self.all.fill_(NAN_WORD)

    def stray(self):
        """Words outside the window that no longer hold NAN_WORD: (count, offset of the first from the window's base)."""
        front, back = self.all[:GUARD] != NAN_WORD, self.all[GUARD + self.words:] != NAN_WORD
        count = int(front.sum()) + int(back.sum())
        if count == 0:
            return 0, None
        return count, (int(front.nonzero()[0]) - GUARD if bool(front.any()) else self.words + int(back.nonzero()[0]))

    def untouched(self):
        return bool((self.all == NAN_WORD).all())


def _bytes_to_words(nbytes):
    assert nbytes % 4 == 0, nbytes
    return nbytes // 4


class Call:
    """The buffers of one forward + backward call: inputs hold the problem's values, outputs the poison."""

    def __init__(self, c, prob, saved_bytes, scratch_bytes, device):
        self.device = device
        self.inputs, self.outputs = {}, {}               # name -> Guarded
        first = c.n_first if c.n_first else c.n
        self.x_first = self._input("x_first", prob.x[:first])
        self.x_rest = self._input("x_rest", prob.x[first:]) if c.n_first else None
        self.params = [self._input(name, prob.p[name]) for name in NAMES]
        self.dz = self._input("dz", prob.dz)
        self.z = self._output("z", prob.dz.shape)
        self.grads = [self._output("grad " + name, prob.p[name].shape) for name in NAMES]
        self.saved = self.outputs["saved"] = Guarded(_bytes_to_words(saved_bytes), device)
        self.scratch = self.outputs["scratch"] = Guarded(_bytes_to_words(scratch_bytes), device)
        self.stray_after_forward = {}
        self.changed_after_forward = []
        self._originals = {name: g.all.clone() for name, g in self.inputs.items()}

    def _input(self, name, values):
        g = self.inputs[name] = Guarded(values.numel(), self.device)
        view = g.f32.view(values.shape)
        view.copy_(values)
        return view

    def _output(self, name, shape):
        g = self.outputs[name] = Guarded(math.prod(shape), self.device)
        return g.f32.view(shape)

    def inputs_changed(self):
        return [name for name, g in self.inputs.items() if not torch.equal(g.all, self._originals[name])]

    def strays(self):
        found = {name: g.stray() for name, g in self.outputs.items()}
        return {name: s for name, s in found.items() if s[0]}

    def after_forward(self):
        """What the forward call alone is held to; scratch is scratch, so it is poisoned again before the backward."""
        self.stray_after_forward = self.strays()
        self.changed_after_forward = self.inputs_changed()
        self.scratch.poison()


# ------------------------------------------------------------------------------------------------------------------ checker
def rel_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def assert_close(got, ref, tol, what="", book=None):
    """Every element finite; |got - ref|_inf <= tol * |ref|_inf AND, element by element, |got - ref| <= atol + rtol * |ref| with
    atol = tol * |ref|_inf and rtol = 64 * tol.  book = (case, quantity): where the error is kept for the module's report (before
    anything is asserted)."""
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    finite = torch.isfinite(g)
    e = rel_err(g, r) if bool(finite.all()) else float("inf")
    if book is not None:
        slot = _WORST.setdefault(book[0], {})
        if e > slot.get(book[1], (-1.0, ""))[0]:
            slot[book[1]] = (e, what)
    assert bool(finite.all()), f"{what}: {int((~finite).sum())} of {g.numel()} elements are not finite"
    assert e <= tol, f"{what}: rel err {e:.3e} > {tol:.1e}"
    atol = tol * float(r.abs().max()) + 1e-30
    bad = (g - r).abs() > atol + 64 * tol * r.abs()
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements outside atol {atol:.2e} + {64 * tol:.1e} |ref|"


def check_call(c, call, prob, book=True):
    """Everything a finished forward + backward call is held to (module docstring)."""
    what = _id(c)
    for name, (count, first) in call.stray_after_forward.items():
        assert count == 0, f"{what}: the forward wrote {count} words outside the window of `{name}`, the first at word {first}"
    assert not call.changed_after_forward, f"{what}: the forward wrote to inputs: {call.changed_after_forward}"
    for name, (count, first) in call.strays().items():
        words = call.outputs[name].words
        assert count == 0, f"{what}: {count} words outside the window of `{name}` ({words} words) were written, the first at word {first}"
    changed = call.inputs_changed()
    assert not changed, f"{what}: inputs were written: {changed}"
    bk = (lambda q: (what, q)) if book else (lambda q: None)
    assert_close(call.z, prob.z, TOL_Z, f"{what} z", book=bk("z"))
    for name, g in zip(NAMES, call.grads):
        assert_close(g, prob.grads[name], TOL_GRAD, f"{what} grad {name[len(PREFIX):]}", book=bk("grad"))


@pytest.fixture(scope="module", autouse=True)
def _report_worst_errors():
    yield
    if not _WORST:
        return
    print("\nworst relative errors of tests/test_encoder_abi_gpu.py (tolerances: z %.0e, grad %.0e):" % (TOL_Z, TOL_GRAD))
    family = {}
    for case in sorted(_WORST):
        print("  %-36s" % case + "  ".join(f"{q} {_WORST[case][q][0]:.3e} ({_WORST[case][q][1]})" for q in sorted(_WORST[case])))
        for q, (e, _where) in _WORST[case].items():
            slot = family.setdefault(case.split("-")[0], {})
            if e > slot.get(q, (-1.0, ""))[0]:
                slot[q] = (e, case)
    for fam in sorted(family):
        print("  family %-4s" % fam + "  ".join(f"{q} {family[fam][q][0]:.3e} ({family[fam][q][1]})" for q in sorted(family[fam])))


# ---------------------------------------------------------------------------------------------------------- the library call
def _sync():
    torch.cuda.synchronize()
    _lib.check(_lib.load().cpc_async_error_check(_lib.stream_ptr(torch.device(DEV))), "async errors")


def sizes_of(c):
    lib = _lib.load()
    return lib.cpc_encoder_saved_bytes(c.n, c.length, c.hidden), lib.cpc_encoder_scratch_bytes(c.n, c.length, c.hidden)


def run_library(c, call):
    lib = _lib.load()
    st = _lib.stream_ptr(torch.device(DEV))
    first = c.n_first if c.n_first else c.n
    params = _lib.ptr_array(call.params)
    _lib.check(lib.cpc_encoder_forward(_lib.ptr(call.x_first), _lib.ptr(call.x_rest), first, params, _lib.ptr(call.z), _lib.ptr(call.saved.f32),
                                       _lib.ptr(call.scratch.f32), c.n, c.length, c.hidden, EPS, st), "encoder_forward")
    torch.cuda.synchronize()
    call.after_forward()
    _lib.check(lib.cpc_encoder_backward(_lib.ptr(call.x_first), _lib.ptr(call.x_rest), first, params, _lib.ptr(call.dz), _lib.ptr(call.saved.f32),
                                        _lib.ptr(call.scratch.f32), _lib.ptr_array(call.grads), c.n, c.length, c.hidden, EPS, c.deferred, st),
               "encoder_backward")
    if c.deferred:                                          # (call.scratch lives until the join)
        _lib.check(lib.cpc_side_tail_join(st), "side_tail_join")
    _sync()


def _run_case(c, book=True):
    prob = problem_of(c)
    saved_bytes, scratch_bytes = sizes_of(c)
    assert saved_bytes > 0 and scratch_bytes > 0, _lib.load().cpc_last_error().decode()
    call = Call(c, prob, saved_bytes, scratch_bytes, DEV)
    run_library(c, call)
    check_call(c, call, prob, book=book)
    return call


def _assert_same_bits(what, a, b):
    assert torch.equal(a.z.view(torch.int32), b.z.view(torch.int32)), f"{what}: z differs"
    for name, ga, gb in zip(NAMES, a.grads, b.grads):
        assert torch.equal(ga.view(torch.int32), gb.view(torch.int32)), f"{what}: grad {name[len(PREFIX):]} differs"


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_encoder_entry_points_vs_oracle_fp64(case):
    _run_case(case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES_D, ids=_id)
def test_two_input_batches_vs_oracle_fp64_and_the_one_buffer_call(case):
    """D: windows n_first .. n - 1 from x_rest -- held to the oracle, and bit for bit the call with all windows in one buffer."""
    pair = _run_case(case)
    one = _run_case(case._replace(n_first=0), book=False)
    _assert_same_bits(_id(case), pair, one)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES_E, ids=_id)
def test_deferred_backward_vs_oracle_fp64_and_the_plain_backward(case):
    """E: the small passes of conv1-4 on the library's side stream -- held to the oracle, and after the join bit for bit the
    gradients of deferred = 0."""
    deferred = _run_case(case)
    plain = _run_case(case._replace(deferred=0), book=False)
    _assert_same_bits(_id(case), deferred, plain)


# ------------------------------------------------------------------------------------------------------------- F. refusals
#          what,                           hidden, n, length, n_first, x_rest, which passes refuse, the reason cpc_last_error gives
REFUSALS = [("399 samples backward", 256, 2, 399, 2, False, "b", "encoder_backward: inputs shorter than 400 samples are forward-only (got 399)"),
            ("399 samples backward f32 path", 64, 2, 399, 2, False, "b", "encoder_backward: inputs shorter than 400 samples are forward-only (got 399)"),
            ("158 samples", 256, 2, 158, 2, False, "fb", "encoder: 158 samples leave no frame (159 is the shortest input)"),
            ("hidden 48", 48, 2, 400, 2, False, "fb", "encoder: hidden size 48 not supported (32, 64, 128, 256, 512)"),
            ("n_first short without x_rest", 256, 3, 400, 2, False, "fb", "encoder: one input batch holds all n_windows windows (n_first 2 of 3)"),
            ("n_first 0 with x_rest", 256, 3, 400, 0, True, "fb", "encoder: the first batch must hold 1 .. n_windows - 1 windows (got 0 of 3)"),
            ("n_first n with x_rest", 64, 3, 400, 3, True, "fb", "encoder: the first batch must hold 1 .. n_windows - 1 windows (got 3 of 3)")]


@pytest.mark.gpu
@pytest.mark.parametrize("refusal", REFUSALS, ids=[r[0].replace(" ", "-") for r in REFUSALS])
def test_encoder_entry_points_refuse(refusal):
    """A nonzero status with the reason in cpc_last_error; nothing is launched: every word of every buffer keeps the poison; and the
    library works afterwards."""
    what, hidden, n, length, n_first, rest, passes, reason = refusal
    lib = _lib.load()
    st = _lib.stream_ptr(torch.device(DEV))
    if "f" in passes and length < 159 or hidden == 48:
        assert lib.cpc_encoder_saved_bytes(n, length, hidden) == 0 and lib.cpc_encoder_scratch_bytes(n, length, hidden) == 0
        assert reason in lib.cpc_last_error().decode()
    buf = Guarded(1 << 20, DEV)               # (4 MiB: more than either pass of these shapes would touch)
    big = Guarded(1 << 22, DEV)               # saved and scratch: 16 MiB
    pointers = _lib.ptr_array([buf.f32] * 20)
    x_rest = _lib.ptr(buf.f32 if rest else None)
    if "f" in passes:
        status = lib.cpc_encoder_forward(_lib.ptr(buf.f32), x_rest, n_first, pointers, _lib.ptr(buf.f32), _lib.ptr(big.f32), _lib.ptr(big.f32),
                                         n, length, hidden, EPS, st)
        assert status != 0, what
        assert reason in lib.cpc_last_error().decode()
        with pytest.raises(ValueError if status == -1 else RuntimeError, match="encoder_forward"):
            _lib.check(status, "encoder_forward")
    for deferred in (0, 1):
        status = lib.cpc_encoder_backward(_lib.ptr(buf.f32), x_rest, n_first, pointers, _lib.ptr(buf.f32), _lib.ptr(big.f32), _lib.ptr(big.f32),
                                          pointers, n, length, hidden, EPS, deferred, st)
        assert status != 0, what
        assert (reason if length >= 400 else f"forward-only (got {length})") in lib.cpc_last_error().decode()      # (the backward's own floor)
    _lib.check(lib.cpc_side_tail_join(st), "side_tail_join")            # (nothing is pending)
    _sync()
    assert buf.untouched() and big.untouched(), f"{what}: a refused call wrote to its buffers"
    _run_case(_case("F", 256 if hidden % 256 == 0 else 64, 1, 400), book=False)


# ===================================================================================================== no GPU from here on
def test_case_list_reaches_the_paths_it_is_there_for():
    everything = CASES + CASES_D + CASES_E
    assert len({_id(c) for c in everything}) == len(everything)
    assert all(c.length >= 400 and c.hidden in (32, 64, 128, 256, 512) for c in everything)
    # A: the 16 patterns are what the lengths are listed for, at each of the three widths; the plane path has its 64 rows
    assert sorted(EVEN_LENGTHS.values()) == [format(v, "04b") for v in range(16)]
    assert all(400 <= length <= 547 and even_pattern(length) == pattern for length, pattern in EVEN_LENGTHS.items())
    for hidden in (256, 512, 64):
        assert {even_pattern(c.length) for c in CASES_A if c.hidden == hidden} == set(EVEN_LENGTHS.values())
    for c in CASES_A:
        if c.hidden >= 256:
            assert tn_rows(c.n, c.length) >= 64 > tn_rows(c.n - 1, c.length), c
            assert c.n == {2: 16, 3: 13}[frames_after(c.length)[5]]
        else:
            assert c.n == 3
    # B: R of conv4's weight gradient on both sides of 64, and exactly on it
    rows = {(c.n, c.length): tn_rows(c.n, c.length) for c in CASES_B}
    assert rows == {(1, 400): 4, (15, 400): 60, (16, 400): 64, (1, 4800): 32, (2, 4800): 64, (1, 9918): 63, (1, 9919): 64, (1, 9920): 64, (1, 20480): 130}
    assert {c.hidden for c in CASES_B} == {256, 512} and len(CASES_B) == 18
    # (the table of the issue: the fewest windows that give 64 rows)
    for length, n in ((400, 16), (640, 11), (1280, 7), (2560, 4), (4800, 2), (9919, 1)):
        assert tn_rows(n, length) >= 64 > tn_rows(n - 1, length), length
    # C: every width alone, on both sides of the patterns' range and at lengths with many frames
    assert {(c.hidden, c.length) for c in CASES_C} == {(h, l) for h in (32, 64, 128, 256, 512) for l in (400, 479, 547, 3300, 2560)}
    assert all(c.n == 1 for c in CASES_C)
    assert even_pattern(2560) == "1111" and even_pattern(3300) == "1010" and even_pattern(547) == "0001"
    # D: both splits of three windows, on both paths, a mixed pattern each
    assert {(c.hidden, c.length, c.n_first) for c in CASES_D} == {(h, l, f) for h in (256, 128) for l in (404, 539) for f in (1, 2)}
    assert all(c.n == 3 and 0 < c.n_first < c.n for c in CASES_D) and {even_pattern(c.length) for c in CASES_D} == {"0110", "1001"}
    # E: four shapes of A and the one that sits on R = 64
    assert all(c.deferred == 1 and c.hidden in (256, 512) for c in CASES_E)
    assert sum(_shape_key(c) in {_shape_key(a) for a in CASES_A} for c in CASES_E) == 4
    assert any((c.hidden, c.n, c.length) == (512, 2, 4800) for c in CASES_E)
    assert {even_pattern(c.length) for c in CASES_E} >= {"0000", "0110", "1111", "1001"}
    # the f32 path's two-product branch is tests/test_gpu_parity.py::test_encoder_vs_oracle_fp64's (32, 512, 2560), not this file's
    assert not any(two_product_layers(c.hidden, c.n, c.length) for c in everything)
    assert two_product_layers(32, 512, 2560) == [1] and two_product_layers(64, 505, 2560) == [1]
    assert two_product_layers(32, 504, 2560) == [] and two_product_layers(256, 512, 2560) == []


def test_restated_layout_is_the_library_s():
    """frames_after against cpc_encoder_frames wherever the library is built (the size queries need no GPU)."""
    lib = _lib.load()
    for length in list(range(150, 560)) + [2560, 3300, 4800, 9919, 9920, 19800, 20480]:
        assert frames_after(length)[5] == lib.cpc_encoder_frames(length), length


def encoder_restated(x, p, wrong=None, layer=None):
    """The encoder with its padding written out, so that three of the kernels' possible mistakes can be made at layer `layer`
    (1..4; the mistakes are the host driver's row arithmetic, seen from the values):
      "edge"   backward data: the boundary row t_hi = L_out is dropped -- the last p input rows of every window get no gradient
      "halo"   forward: the halo row in front of every window holds a finite non-zero value (0.01) instead of zero
      "even"   backward data of a layer with L_in > s L_out run on the branch for L_in == s L_out: the boundary row's p outputs
               land on the LAST p input rows instead of rows s L_out - p .. s L_out - 1, which stay as they were (zero)
    wrong = None is the oracle (test_restated_encoder_is_the_oracle).  Returns [N, H, L]."""
    h = x
    for i, (k, s, pad) in enumerate(GEOMETRY):
        l_in = h.shape[2]
        l_out = (l_in + 2 * pad - k) // s + 1
        if wrong in ("edge", "even") and i == layer and h.requires_grad:
            if wrong == "edge":
                assert l_in == s * l_out

                def hook(g, pad=pad):
                    g = g.clone()
                    g[:, :, g.shape[2] - pad:] = 0
                    return g
            else:
                assert l_in > s * l_out

                def hook(g, pad=pad, at=s * l_out):
                    g = g.clone()
                    row = g[:, :, at - pad:at].clone()
                    g[:, :, at - pad:] = 0
                    g[:, :, g.shape[2] - pad:] = row
                    return g
            h = h * 1.0
            h.register_hook(hook)
        padded = torch.nn.functional.pad(h, (pad, pad))
        if wrong == "halo" and i == layer:
            stain = torch.zeros_like(padded)
            stain[:, :, pad - 1] = 0.01
            padded = padded + stain
        u = torch.nn.functional.conv1d(padded, p[f"{PREFIX}conv{i}.weight"], p[f"{PREFIX}conv{i}.bias"], stride=s)
        h = torch.relu(O.channel_norm(u, p[f"{PREFIX}batchNorm{i}.weight"], p[f"{PREFIX}batchNorm{i}.bias"]))
    return h


def run_torch(c, call, prob, wrong=None, layer=None, accumulate=False, past_scratch=False):
    """The call in plain float32 torch on the host: the f32 evaluation of the oracle (wrong = None), or encoder_restated with one of
    its mistakes; accumulate: the gradients are added to what the buffers hold; past_scratch: one word behind `scratch` is written."""
    forward_fn = None if wrong is None else functools.partial(encoder_restated, wrong=wrong, layer=layer)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)          # (torch's threaded f32 conv backward on the host: see the module docstring)
    try:
        z, grads = differentiate(prob.x, prob.p, prob.dz, torch.float32, check_margin=False, forward_fn=forward_fn)
    finally:
        torch.set_num_threads(threads)
    call.z.copy_(z)
    call.saved.f32.zero_()
    call.scratch.f32.zero_()
    call.after_forward()
    for name, g in zip(NAMES, call.grads):
        if accumulate:
            g += grads[name]
        else:
            g.copy_(grads[name])
    call.scratch.f32.zero_()
    if past_scratch:
        call.scratch.all[GUARD + call.scratch.words] = 0


MIXED, EVEN, SPLIT = _case("A", 64, 3, 404), _case("A", 64, 3, 479), _case("D", 128, 3, 539, n_first=1)
assert MIXED in CASES and EVEN in CASES and SPLIT in CASES_D


def _host_call(c):
    prob = problem_of(c)
    return prob, Call(c, prob, 4096, 8192, "cpu")


@pytest.mark.parametrize("case", [MIXED, EVEN, SPLIT, _case("C", 32, 1, 547), _case("B", 256, 1, 400)], ids=_id)
def test_harness_accepts_the_f32_evaluation_of_the_oracle(case):
    prob, call = _host_call(case)
    with pytest.raises(AssertionError, match="not finite"):
        check_call(case, call, prob, book=False)                    # nothing written yet: NaN inside every window
    run_torch(case, call, prob)
    check_call(case, call, prob, book=False)


def test_restated_encoder_is_the_oracle():
    for c in (MIXED, EVEN):
        prob = problem_of(c)
        p64 = {k: v.double() for k, v in prob.p.items()}
        ref = oracle_forward(prob.x.double(), p64)
        assert rel_err(encoder_restated(prob.x.double(), p64).permute(0, 2, 1), ref) < 1e-13
        assert rel_err(ref, prob.z) == 0.0


# 404 samples: layers 1..4 are 0110 -- layer 1 (81 -> 20) and 4 (5 -> 2) are not even, 2 and 3 are;  479: all four are even
@pytest.mark.parametrize("case,mistake", [(MIXED, dict(wrong="edge", layer=2)), (MIXED, dict(wrong="edge", layer=3)), (EVEN, dict(wrong="edge", layer=1)),
                                          (EVEN, dict(wrong="edge", layer=4)), (MIXED, dict(wrong="halo", layer=1)), (EVEN, dict(wrong="halo", layer=4)),
                                          (MIXED, dict(wrong="even", layer=4)), (MIXED, dict(wrong="even", layer=1)), (EVEN, dict(accumulate=True)),
                                          (MIXED, dict(past_scratch=True))],
                         ids=lambda v: _id(v) if isinstance(v, Case) else "-".join(f"{k}-{w}" for k, w in v.items()))
def test_harness_rejects_wrong_implementations(case, mistake):
    prob, call = _host_call(case)
    run_torch(case, call, prob, **mistake)
    with pytest.raises(AssertionError) as info:
        check_call(case, call, prob, book=False)
    expected = {"accumulate": "not finite", "past_scratch": "outside the window of `scratch`", "wrong": "rel err"}[next(iter(mistake))]
    assert expected in str(info.value), info.value


def test_harness_rejects_what_only_the_forward_did_and_a_changed_input():
    prob, call = _host_call(MIXED)
    call.scratch.all[GUARD - 1] = 0                                 # the forward writes in front of its scratch; the refill hides it later
    run_torch(MIXED, call, prob)
    with pytest.raises(AssertionError, match="the forward wrote 1 words outside the window of `scratch`, the first at word -1"):
        check_call(MIXED, call, prob, book=False)
    prob, call = _host_call(MIXED)
    run_torch(MIXED, call, prob)
    call.dz[0, 0, 0] += 1.0
    with pytest.raises(AssertionError, match="inputs were written"):
        check_call(MIXED, call, prob, book=False)
