"""cpc_transformer_forward / cpc_transformer_backward over the whole domain tr_layout (cpc2_amd/csrc/transformer.hip) accepts:
every width 32 .. 512 (head sizes 4 .. 64), d_out != d_model, sizeSeq 1 .. 128 on both attention families (the generic
kernels and the MFMA kernels of head size 32), 1 .. 4 stacked layers in ONE call, 1 .. 64 classifiers, Krelpos == NULL,
dx == NULL, deferred 0 / 1, Q|K|V weights and gradients back to back or apart -- and everything it refuses.

Reference: oracle.cpc_oracle.transformer_layer_forward in fp64, layer by layer, differentiated by autograd; parameters from
oracle.synth.transformer_params, every layer's ReLU decisions settled on that layer's fp64 input (oracle/settle.py; every
oracle run asserts that no pre-activation lies within RELU_MARGIN of zero).  No element is excluded from any comparison.

Harness.  Every buffer of a call -- x, dout, each parameter, out, dx, each gradient, saved, scratch -- is a window of a larger
allocation filled with ONE quiet-NaN bit pattern (NAN_WORD), and the windows of out, dx, the gradients, saved and scratch hold
that pattern too when the forward call starts; scratch is filled again between forward and backward.  Afterwards
  * every word outside the windows (the tensor shapes of include/cpc2_hip.h; exactly cpc_transformer_saved_bytes /
    _scratch_bytes) is compared as int32 and must be unchanged, the inputs bit for bit;
  * every element of out, dx and each gradient is finite and within the project's tolerances (tests/test_gpu_parity.py:
    out 2e-5, dx 1e-4, gradients 2e-4 of the reference's largest element, and element by element atol + 64 tol |ref|).
So the library stays inside the sizes it reports, never uses scratch or saved state it did not write (a NaN would reach an
output), keeps nothing in scratch between the passes, and overwrites the gradients (NaN + g is NaN).  Nothing relies on a fault.
Every case ends with cpc_async_error_check.

The unmarked tests at the end need no GPU: the checker accepts the f32 evaluation of the oracle and rejects five wrong
implementations, and the case list is held to the paths it is there to reach.

Worst relative errors per family, measured on an MI355X (python -m pytest tests/test_transformer_abi_gpu.py -s prints the
table per case), against out 2e-5 / dx 1e-4 / grad 2e-4:
  family                                            out        dx         grad       worst case (out / dx / grad)
  A  head sizes, sizeSeq edges, Krelpos NULL        6.8e-07    7.8e-07    1.0e-06    d512 ss31 / d256 ss2 / abspos module d256 ss97
  B  d_out != d_model, classifier heads             6.1e-07    7.2e-07    1.2e-06    256->64 nc12 ss116 / 256->512 / 256->64 nc12 ss116
  C  2 - 4 stacked layers, dx NULL, deferred        7.7e-07    7.1e-07    1.5e-06    d512 ss40 2 layers (all three)
  D  Q|K|V and their gradients packed / apart       5.2e-07    4.1e-07    5.3e-07    d256 ss33 (the four forms give the same figures)
  E  training mode                                  6.9e-07    7.9e-07    1.1e-06    d256 ss97 3 layers (all three)
The 3- and 4-layer calls, where rounding compounds through the LayerNorms (f32-torch evaluation of the oracle against the fp64
oracle | the kernels against the fp64 oracle; plain, dx == NULL and deferred give the same figures):
  case                                f32 oracle: out / dx / grad          kernels: out / dx / grad
  C d256 ss97, 3 layers               6.2e-07 / 6.2e-07 / 1.2e-06          6.0e-07 / 5.0e-07 / 9.6e-07
  C d256 ss97, 4 layers               6.9e-07 / 7.6e-07 / 1.3e-06          5.8e-07 / 5.9e-07 / 1.1e-06
  C d64 ss33 s66, 4 layers            5.6e-07 / 5.6e-07 / 1.5e-06          3.3e-07 / 3.4e-07 / 7.4e-07
  C d128 ss65, 3 layers               4.7e-07 / 5.7e-07 / 9.0e-07          3.9e-07 / 4.3e-07 / 8.0e-07
  E d256 ss97, 3 layers, p = 0.1      7.9e-07 / 6.7e-07 / 1.3e-06          6.9e-07 / 7.9e-07 / 1.1e-06
The project tolerances hold on all of them with a factor of 25 to spare, so no case has a bound of its own.
"""
import collections
import functools
import math

import pytest
import torch

from cpc2_amd import _lib
from oracle import cpc_oracle as O
from oracle import dropmask as D
from oracle import synth
from oracle.settle import RELU_MARGIN, settle_relu_decisions

DEV = "cuda:0"
NAN_WORD = 0x7FC0BEEF              # the one bit pattern of every poisoned word: a quiet NaN no arithmetic produces
GUARD = 64                         # words of poison before and behind every window (256 bytes: the windows keep torch's alignment)
P_DROP = 0.1
TOL_OUT, TOL_DX, TOL_GRAD = 2e-5, 1e-4, 2e-4          # tests/test_gpu_parity.py::test_transformer_vs_oracle_fp64

# the 15 tensors of a layer in the C ABI's order (include/cpc2_hip.h)
ABI = ["multihead.Wq.weight", "multihead.Wk.weight", "multihead.Wv.weight", "multihead.Wo.weight", "multihead.Att.Krelpos",
       "ln_multihead.weight", "ln_multihead.bias", "ffnetwork.lin1.weight", "ffnetwork.lin1.bias", "ffnetwork.lin2.weight",
       "ffnetwork.lin2.bias", "last_linear.weight", "last_linear.bias", "ln_ffnetwork.weight", "ln_ffnetwork.bias"]
KREL = 4

_WORST = {}         # case id -> {"out" | "dx" | "grad": (worst relative error, where)}


# ----------------------------------------------------------------------------------------------------------------- the cases
# d -> dout, blocks of ss frames in s frames, n samples, `layers` layers in one call, nc classifiers in the last one's head.
# krel: relative positions (False: Krelpos == NULL and grads[Krelpos] == NULL);  dx False: dx == NULL;  deferred: the ABI's flag;
# p: dropout (0: eval mode);  wpack / gpack: Wq|Wk|Wv, resp. their three gradients, back to back in one allocation.
Case = collections.namedtuple("Case", "family d dout ss s n layers nc krel dx deferred p wpack gpack")


def _case(family, d, ss, s, dout=None, n=2, layers=1, nc=1, krel=True, dx=True, deferred=0, p=0.0, wpack=True, gpack=True):
    return Case(family, d, dout or d, ss, s, n, layers, nc, krel, dx, deferred, p, wpack, gpack)


def _id(c):
    parts = [c.family, f"d{c.d}" + (f"to{c.dout}" if c.dout != c.d else ""), f"ss{c.ss}", f"s{c.s}"]
    parts += [f"n{c.n}"] if c.n != 2 else []
    parts += [f"layers{c.layers}"] if c.layers != 1 else []
    parts += [f"nc{c.nc}"] if c.nc != 1 else []
    parts += [] if c.krel else ["nokrel"]
    parts += [] if c.dx else ["nodx"]
    parts += ["deferred"] if c.deferred else []
    parts += ["train"] if c.p > 0 else []
    if c.family == "D":
        parts += ["w-" + ("packed" if c.wpack else "apart"), "g-" + ("packed" if c.gpack else "apart")]
    return "-".join(parts)


# A. head sizes and sizeSeq edges, one layer, d_out = d_model
CASES_A = (
    # d = 128: head size 16, attn_bwd_kernel<8>, RowCfg<128>
    [_case("A", 128, ss, s) for ss, s in ((128, 128), (33, 66), (1, 3))]
    # d = 64: head size 8; (128, 128): four query tiles through the backward
    + [_case("A", 64, ss, s) for ss, s in ((128, 128), (97, 97), (7, 21))]
    # d = 512: head size 64, the generic kernels' LDS at its largest
    + [_case("A", 512, 65, 65), _case("A", 512, 31, 62), _case("A", 512, 1, 1, n=1)]
    # d = 32: head size 4
    + [_case("A", 32, 128, 128), _case("A", 32, 63, 63)]
    # d = 256: the MFMA kernels, a wave owns 32 query rows: no full tile, one row in the last wave, one row short of a tile
    + [_case("A", 256, ss, s) for ss, s in ((1, 5), (2, 2), (31, 31), (33, 99), (63, 63), (64, 64), (65, 65), (95, 95), (97, 97),
                                             (115, 115), (127, 127))]
    # Krelpos == NULL: the MFMA kernels skip the R tiles; the generic kernels at head size 16
    + [_case("A", 256, 128, 128, krel=False), _case("A", 256, 97, 97, krel=False), _case("A", 128, 33, 66, krel=False)]
)
# B. rectangular d_out, one layer; the multi-classifier head
CASES_B = (
    [_case("B", d, 40, 40, dout=dout) for d, dout in ((256, 64), (64, 256), (512, 32), (32, 512), (128, 256), (256, 512))]
    + [_case("B", 64, 33, 33, dout=128, nc=3), _case("B", 256, 116, 116, dout=64, nc=12, n=1), _case("B", 32, 8, 8, nc=64),
       _case("B", 128, 65, 65, nc=2)]
)
# C. stacked layers in one call, each shape plain, with dx == NULL and with deferred = 1
_SHAPES_C = [dict(d=256, ss=97, s=97, layers=2), dict(d=256, ss=97, s=97, layers=3), dict(d=256, ss=97, s=97, layers=4),
             dict(d=64, ss=33, s=66, layers=4), dict(d=512, ss=40, s=40, layers=2), dict(d=128, ss=65, s=65, layers=3),
             dict(d=64, ss=32, s=32, layers=2, nc=3)]
CASES_C = [_case("C", **shape, **way) for shape in _SHAPES_C for way in (dict(), dict(dx=False), dict(deferred=1))]
# D. argument forms: both branches of the contiguity tests in forward, backward-weights and backward-data
CASES_D = [_case("D", d, ss, s, wpack=wp, gpack=gp) for d, ss, s in ((256, 33, 33), (64, 32, 64)) for wp in (True, False)
           for gp in (True, False)]
# E. training mode on the new paths; layer l of a stacked call under seed + 0x1000 * l
CASES_E = [_case("E", 128, 33, 66, p=P_DROP), _case("E", 256, 65, 65, p=P_DROP), _case("E", 256, 40, 40, dout=64, p=P_DROP),
           _case("E", 256, 97, 97, layers=3, p=P_DROP)]
CASES = CASES_A + CASES_B + CASES_C + CASES_D + CASES_E

def tolerances(c):
    """The project's numbers, for every case.  (For the 3- and 4-layer calls, where rounding compounds through the LayerNorms, the
    bound would be max(project number, 4 x the error of the f32-torch evaluation of the oracle against fp64); that evaluation is
    off by 8e-7 / 8e-7 / 1.5e-6 at most on those cases (module docstring), so the project numbers are the bound there too.)"""
    return dict(out=TOL_OUT, dx=TOL_DX, grad=TOL_GRAD)


# ------------------------------------------------------------------------------------------------------ values and references
Problem = collections.namedtuple("Problem", "p x gout seed masks out dx grads")


def _prefix(layer):
    return f"L{layer}."


def _seeds(c):
    k = 7919 * c.d + 131 * c.dout + 17 * c.ss + 3 * c.s + 1009 * c.layers + 53 * c.nc + (0 if c.krel else 5) + (11 if c.p > 0 else 0)
    return k, 0x5EED00000000 + k if c.p > 0 else 0


def oracle_forward(x, p, c, masks, check_margin=True, layer_fn=None):
    """The stacked layers of c in the dtype of x and p, the classifiers in the last one."""
    h = x
    for l in range(c.layers):
        pre = []
        nc = c.nc if l == c.layers - 1 else 1
        if layer_fn is not None:
            h = layer_fn(h, p, _prefix(l), c.ss)
            continue
        h = O.transformer_layer_forward(h, p, _prefix(l), size_seq=c.ss, n_classifiers=nc, pre_out=pre, drop=masks[l])
        if check_margin:
            assert float(pre[0].abs().min()) >= RELU_MARGIN, f"{_id(c)} layer {l}: a ReLU decision within {RELU_MARGIN} of zero"
    return h


def differentiate(x, p, gout, c, masks, dtype, **kw):
    """(out, dx, {name: gradient}) of sum(out * gout) with everything held in `dtype`."""
    pd = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in p.items()}      # (clones: the problem's tensors are shared)
    xd = x.detach().clone().to(dtype).requires_grad_(True)
    out = oracle_forward(xd, pd, c, masks, **kw)
    (out * gout.to(dtype)).sum().backward()
    return out.detach(), xd.grad, {k: v.grad for k, v in pd.items()}


def _shape_key(c):
    """The fields the values and the reference depend on (not: the argument forms)."""
    return c._replace(family="", dx=True, deferred=0, wpack=True, gpack=True)


@functools.lru_cache(maxsize=3)
def _problem(key):
    c = key
    k, seed = _seeds(c)
    p = {}
    for l in range(c.layers):
        nc = c.nc if l == c.layers - 1 else 1
        p.update(synth.transformer_params(c.d, c.dout, c.ss, 9000 + 10 * k + l, prefix=_prefix(l), n_classifiers=nc))
        if not c.krel:
            del p[_prefix(l) + ABI[KREL]]
    x = synth.features((c.n, c.s, c.d), 9100 + k, relu=True)
    gout = synth.features((c.n, c.s, c.dout) if c.nc == 1 else (c.n, c.s, c.nc, c.dout), 9200 + k)
    masks = [D.layer_masks(seed, c.n, c.s, c.ss, c.p, layer=l) if c.p > 0 else None for l in range(c.layers)]
    h = x.double()
    for l in range(c.layers):                # every layer's decisions on ITS fp64 input, under its masks
        nc = c.nc if l == c.layers - 1 else 1
        settle_relu_decisions(p, _prefix(l), h, n_classifiers=nc, size_seq=c.ss, drop=masks[l])
        if l + 1 < c.layers:
            with torch.no_grad():
                h = O.transformer_layer_forward(h, {n_: v.double() for n_, v in p.items()}, _prefix(l), size_seq=c.ss, drop=masks[l])
    return Problem(p, x, gout, seed, masks, *differentiate(x, p, gout, c, masks, torch.float64))


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


def _bytes_to_words(nbytes):
    assert nbytes % 4 == 0, nbytes
    return nbytes // 4


class Call:
    """The buffers of one forward + backward call.  params / grads: per layer the 15 tensors in ABI order (None: absent), views
    of Guarded allocations; inputs hold the problem's values, outputs the poison."""

    def __init__(self, c, prob, saved_bytes, scratch_bytes, device):
        self.device = device
        self.inputs, self.outputs = {}, {}               # name -> Guarded
        self.x = self._input("x", prob.x)
        self.gout = self._input("dout", prob.gout)
        self.params, self.grads, self.grad_names = [], [], []
        for l in range(c.layers):
            names = [_prefix(l) + a for a in ABI]
            tensors = [prob.p.get(name) for name in names]
            row, grow = [None] * len(ABI), [None] * len(ABI)
            if c.wpack:
                d2 = c.d * c.d
                g = self.inputs[_prefix(l) + "Wq|Wk|Wv"] = Guarded(3 * d2, device)
                for i in range(3):
                    row[i] = g.f32[i * d2:(i + 1) * d2].view(c.d, c.d)
                    row[i].copy_(tensors[i])
            if c.gpack:
                d2 = c.d * c.d
                g = self.outputs["grad " + _prefix(l) + "Wq|Wk|Wv"] = Guarded(3 * d2, device)
                for i in range(3):
                    grow[i] = g.f32[i * d2:(i + 1) * d2].view(c.d, c.d)
            for i, (name, t) in enumerate(zip(names, tensors)):
                if t is None:
                    continue
                if row[i] is None:
                    row[i] = self._input(name, t)
                if grow[i] is None:
                    grow[i] = self._output("grad " + name, t.shape)
            self.params.append(row)
            self.grads.append(grow)
            self.grad_names.append(names)
        out_shape = (c.n, c.s, c.dout) if c.nc == 1 else (c.n, c.s, c.nc, c.dout)
        self.out = self._output("out", out_shape)
        self.dx = self._output("dx", (c.n, c.s, c.d)) if c.dx else None
        self.saved = self.outputs["saved"] = Guarded(_bytes_to_words(saved_bytes), device)
        self.scratch = self.outputs["scratch"] = Guarded(_bytes_to_words(scratch_bytes), device)
        self.scratch_stray_after_forward = (0, None)
        self._originals = {name: g.all.clone() for name, g in self.inputs.items()}
        if c.wpack:
            assert all(r[1].data_ptr() == r[0].data_ptr() + 4 * c.d * c.d and r[2].data_ptr() == r[1].data_ptr() + 4 * c.d * c.d for r in self.params)
        else:
            assert all(r[1].data_ptr() != r[0].data_ptr() + 4 * c.d * c.d for r in self.params)
        if c.gpack:
            assert all(r[1].data_ptr() == r[0].data_ptr() + 4 * c.d * c.d and r[2].data_ptr() == r[1].data_ptr() + 4 * c.d * c.d for r in self.grads)
        else:
            assert all(r[1].data_ptr() != r[0].data_ptr() + 4 * c.d * c.d for r in self.grads)

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


# ------------------------------------------------------------------------------------------------------------------ checker
def rel_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def assert_close(got, ref, tol, what="", book=None):
    """(tests/test_transformer_dropout_gpu.py) every element finite; |got - ref|_inf <= tol * |ref|_inf AND, element by element,
    |got - ref| <= atol + rtol * |ref| with atol = tol * |ref|_inf and rtol = 64 * tol.  book = (case, quantity): where the error
    is kept for the module's report (before anything is asserted)."""
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
    count, first = call.scratch_stray_after_forward
    assert count == 0, f"{what}: the forward wrote {count} words outside its scratch window, the first at word {first}"
    for name, g in call.outputs.items():
        count, first = g.stray()
        assert count == 0, f"{what}: {count} words outside the window of `{name}` ({g.words} words) were written, the first at word {first}"
    changed = call.inputs_changed()
    assert not changed, f"{what}: inputs were written: {changed}"
    tol = tolerances(c)
    bk = (lambda q: (what, q)) if book else (lambda q: None)
    assert_close(call.out, prob.out, tol["out"], f"{what} out", book=bk("out"))
    if c.dx:
        assert_close(call.dx, prob.dx, tol["dx"], f"{what} dx", book=bk("dx"))
    for l in range(c.layers):
        for i, name in enumerate(call.grad_names[l]):
            if name not in prob.p:
                assert i == KREL and not c.krel and call.grads[l][i] is None
                continue
            assert_close(call.grads[l][i], prob.grads[name], tol["grad"], f"{what} grad {name}", book=bk("grad"))


@pytest.fixture(scope="module", autouse=True)
def _report_worst_errors():
    yield
    if not _WORST:
        return
    print("\nworst relative errors of tests/test_transformer_abi_gpu.py (tolerances: out %.0e, dx %.0e, grad %.0e):"
          % (TOL_OUT, TOL_DX, TOL_GRAD))
    family = {}
    for case in sorted(_WORST):
        print("  %-44s" % case + "  ".join(f"{q} {_WORST[case][q][0]:.3e} ({_WORST[case][q][1]})" for q in sorted(_WORST[case])))
        for q, (e, _where) in _WORST[case].items():
            slot = family.setdefault(case.split("-")[0], {})
            if e > slot.get(q, (-1.0, ""))[0]:
                slot[q] = (e, case)
    for fam in sorted(family):
        print("  family %-4s" % fam + "  ".join(f"{q} {family[fam][q][0]:.3e} ({family[fam][q][1]})" for q in sorted(family[fam])))


# ---------------------------------------------------------------------------------------------------------- the library call
def _flat(rows):
    return [t for row in rows for t in row]


def _sync():
    torch.cuda.synchronize()
    _lib.check(_lib.load().cpc_async_error_check(_lib.stream_ptr(torch.device(DEV))), "async errors")


def sizes_of(c):
    lib = _lib.load()
    args = (c.n, c.s, c.d, c.dout, c.ss, c.layers, c.nc)
    return lib.cpc_transformer_saved_bytes(*args), lib.cpc_transformer_scratch_bytes(*args)


def run_library(c, call, seed):
    lib = _lib.load()
    st = _lib.stream_ptr(torch.device(DEV))
    dims = (c.n, c.s, c.d, c.dout, c.ss, c.layers, c.nc)
    params = _lib.ptr_array(_flat(call.params))
    _lib.check(lib.cpc_transformer_forward(_lib.ptr(call.x), params, _lib.ptr(call.out), _lib.ptr(call.saved.f32), _lib.ptr(call.scratch.f32),
                                           *dims, c.p, seed, st), "transformer_forward")
    torch.cuda.synchronize()
    call.scratch_stray_after_forward = call.scratch.stray()
    call.scratch.poison()                                   # scratch is scratch: nothing may survive in it
    _lib.check(lib.cpc_transformer_backward(_lib.ptr(call.x), params, _lib.ptr(call.gout), _lib.ptr(call.saved.f32), _lib.ptr(call.scratch.f32),
                                            _lib.ptr(call.dx), _lib.ptr_array(_flat(call.grads)), *dims, c.p, seed, c.deferred, st),
               "transformer_backward")
    if c.deferred:                                          # (call.scratch lives until the join)
        _lib.check(lib.cpc_side_tail_join(st), "side_tail_join")
    _sync()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_transformer_entry_points_vs_oracle_fp64(case):
    prob = problem_of(case)
    saved_bytes, scratch_bytes = sizes_of(case)
    assert saved_bytes > 0 and scratch_bytes > 0, _lib.load().cpc_last_error().decode()
    call = Call(case, prob, saved_bytes, scratch_bytes, DEV)
    run_library(case, call, prob.seed)
    check_call(case, call, prob)


# ----------------------------------------------------------------------------------------------------- through the modules
def _run_module(net, layer, prob, prefix=_prefix(0)):
    sd = layer.state_dict()
    sd.update({k[len(prefix):]: v for k, v in prob.p.items()})
    layer.load_state_dict(sd)
    net = net.to(DEV).eval()
    xd = prob.x.to(DEV).requires_grad_(True)
    out = net(xd)
    (out * prob.gout.to(DEV)).sum().backward()
    _sync()
    return out.detach().cpu(), xd.grad.cpu(), {prefix + name: prm.grad.cpu() for name, prm in layer.named_parameters()}


def _compare_module(what, got, ref):
    (out, dx, grads), (ref_out, ref_dx, ref_grads) = got, ref
    assert_close(out, ref_out, TOL_OUT, f"{what} out", book=(what, "out"))
    assert_close(dx, ref_dx, TOL_DX, f"{what} dx", book=(what, "dx"))
    assert set(grads) == set(ref_grads)
    for name in sorted(grads):
        assert_close(grads[name], ref_grads[name], TOL_GRAD, f"{what} grad {name}", book=(what, "grad"))


@pytest.mark.gpu
def test_rectangular_layer_through_the_module():
    """buildTransformerAR(dimEncoded = 64, dimAR = 256, ...): d_model 256 -> d_out 64, the values of the ABI case."""
    from cpc2_amd.transformers import buildTransformerAR
    c = _case("B", 256, 40, 40, dout=64)
    prob = problem_of(c)
    net = buildTransformerAR(64, 256, 1, 40, False)
    _compare_module("B-module-d256to64-ss40", _run_module(net, net[0], prob), (prob.out, prob.dx, prob.grads))


@pytest.mark.gpu
def test_abspos_module_at_the_mfma_width():
    """buildTransformerAR(256, 256, 1, 97, abspos = True): the position table in front, Krelpos == NULL on the MFMA kernels."""
    from cpc2_amd.transformers import buildTransformerAR
    c = _case("A", 256, 97, 97, krel=False)
    k, _seed = _seeds(c)
    net = buildTransformerAR(256, 256, 1, 97, True)
    pe = net[0].pe[:, :c.s].double()             # as the module holds it (computed in fp32 by torch): the oracle adds the same
    p = synth.transformer_params(c.d, c.dout, c.ss, 9500 + k, prefix=_prefix(0))
    del p[_prefix(0) + ABI[KREL]]
    x = synth.features((c.n, c.s, c.d), 9600 + k, relu=True)
    gout = synth.features((c.n, c.s, c.dout), 9700 + k)
    settle_relu_decisions(p, _prefix(0), x.double() + pe, size_seq=c.ss)
    p64 = {k_: v.double().requires_grad_(True) for k_, v in p.items()}
    x64 = x.double().requires_grad_(True)
    out = oracle_forward(x64 + pe, p64, c, [None])
    (out * gout.double()).sum().backward()
    prob = Problem(p, x, gout, 0, [None], out.detach(), x64.grad, {k_: v.grad for k_, v in p64.items()})
    _compare_module("A-module-abspos-d256-ss97", _run_module(net, net[1], prob), (prob.out, prob.dx, prob.grads))


# ------------------------------------------------------------------------------------------------------------- F. refusals
#          what,                    n, s, d, dout, ss, layers, nc, the reason cpc_last_error gives
REFUSALS = [("d_model 96", 2, 32, 96, 96, 32, 1, 1, "model dims 96/96 not supported"),
            ("d_out 48", 2, 32, 64, 48, 32, 1, 1, "model dims 64/48 not supported"),
            ("size_seq 129", 2, 129, 64, 64, 129, 1, 1, "need 0 < sizeSeq <= 128 (got 129)"),
            ("size_seq 0", 2, 32, 64, 64, 0, 1, 1, "need 0 < sizeSeq <= 128 (got 0)"),
            ("s not a multiple of size_seq", 2, 50, 64, 64, 32, 1, 1, "sequence length 50 must be a multiple of sizeSeq 32"),
            ("layers 0", 2, 32, 64, 64, 32, 0, 1, "1..4 layers supported (got 0)"),
            ("layers 5", 2, 32, 64, 64, 32, 5, 1, "1..4 layers supported (got 5)"),
            ("nc 0", 2, 32, 64, 64, 32, 1, 0, "1..64 classifiers in the last layer's head (got 0)"),
            ("nc 65", 2, 32, 64, 64, 32, 1, 65, "1..64 classifiers in the last layer's head (got 65)"),
            ("stacked layers with d_out != d_model", 2, 32, 64, 128, 32, 2, 1, "stacked layers need dmodel == dout")]


@pytest.mark.gpu
@pytest.mark.parametrize("refusal", REFUSALS, ids=[r[0].replace(" ", "-") for r in REFUSALS])
def test_transformer_entry_points_refuse_what_tr_layout_refuses(refusal):
    """Both size queries return 0, both entry points a nonzero status with the reason in cpc_last_error; nothing is launched."""
    what, reason = refusal[0], refusal[-1]
    dims = refusal[1:-1]
    lib = _lib.load()
    st = _lib.stream_ptr(torch.device(DEV))
    assert lib.cpc_transformer_saved_bytes(*dims) == 0 and lib.cpc_transformer_scratch_bytes(*dims) == 0
    assert reason in lib.cpc_last_error().decode()
    buf = Guarded(1 << 16, DEV)
    layers = max(1, dims[5])
    pointers = _lib.ptr_array([buf.f32] * (len(ABI) * layers))
    status = lib.cpc_transformer_forward(_lib.ptr(buf.f32), pointers, _lib.ptr(buf.f32), _lib.ptr(buf.f32), _lib.ptr(buf.f32), *dims, 0.0, 0, st)
    assert status != 0, what
    assert reason in lib.cpc_last_error().decode()
    with pytest.raises(ValueError if status == -1 else RuntimeError, match="transformer"):
        _lib.check(status, "transformer_forward")
    for deferred in (0, 1):
        status = lib.cpc_transformer_backward(_lib.ptr(buf.f32), pointers, _lib.ptr(buf.f32), _lib.ptr(buf.f32), _lib.ptr(buf.f32), _lib.ptr(buf.f32),
                                              pointers, *dims, 0.0, 0, deferred, st)
        assert status != 0, what
        assert reason in lib.cpc_last_error().decode()
    _lib.check(lib.cpc_side_tail_join(st), "side_tail_join")            # (nothing is pending)
    _sync()
    assert bool((buf.all.cpu() == NAN_WORD).all()), f"{what}: a refused call wrote to its buffers"


@pytest.mark.gpu
def test_module_refuses_a_width_the_kernels_do_not_have():
    from cpc2_amd.transformers import TransformerLayer
    layer = TransformerLayer(sizeSeq=32, dmodel=96, dout=96).to(DEV).eval()
    x = torch.zeros(2, 32, 96, device=DEV)
    with pytest.raises(ValueError, match="model dims 96/96 not supported"):
        layer(x)
    _sync()


# ===================================================================================================== no GPU from here on
def _attention_family(c):
    return "mfma" if c.d // 8 == 32 else "generic"


def test_case_list_reaches_the_paths_it_is_there_for():
    assert len({_id(c) for c in CASES}) == len(CASES)
    assert {c.d // 8 for c in CASES} >= {4, 8, 16, 32, 64}
    for family in ("generic", "mfma"):
        mine = [c for c in CASES if _attention_family(c) == family]
        for rows in (32, 64, 96):                       # the query tiles of both families hold 32 rows
            assert any(c.ss < rows for c in mine) and any(c.ss == rows + 1 for c in mine), (family, rows)
        assert any(c.ss % 2 == 1 and c.krel for c in mine)          # Krelpos rows off 16-byte alignment
        assert any(not c.krel for c in mine), family
        assert any(c.s > c.ss for c in mine), family                 # more than one block per sample
        assert any(c.p > 0 for c in mine), family
    assert any(c.ss == 128 for c in CASES if _attention_family(c) == "generic") and any(c.ss == 1 for c in CASES)
    assert {c.layers for c in CASES} == {1, 2, 3, 4}
    assert {c.nc for c in CASES} >= {1, 2, 64}
    assert any(c.dout < c.d for c in CASES) and any(c.dout > c.d for c in CASES)
    for shape in {_shape_key(c) for c in CASES_C}:                   # each stacked shape plain, without dx and deferred
        ways = {(c.dx, c.deferred) for c in CASES_C if _shape_key(c) == shape}
        assert ways == {(True, 0), (False, 0), (True, 1)}, shape
    assert any(c.nc > 1 and c.deferred for c in CASES_C) and any(c.nc > 1 and c.layers > 1 for c in CASES_C)
    for d in (256, 64):                                              # both contiguity branches, crossed
        assert {(c.wpack, c.gpack) for c in CASES_D if c.d == d} == {(True, True), (True, False), (False, True), (False, False)}
    assert all(c.layers == 1 or c.d == c.dout for c in CASES)
    assert all(c.s % c.ss == 0 and 1 <= c.ss <= 128 for c in CASES)


def layer_restated(x, p, prefix, ss, wrong=None):
    """One layer (one classifier, eval mode) written out with explicit index arithmetic, so that three mistakes can be made:
      "relpos+1"   the relative-position index S - (i - j) for S - 1 - (i - j)
      "mask"       a causal mask that excludes the diagonal (row 0 keeps its only element)
      "ln2"        the second LayerNorm's moments taken over d_model instead of d_out
    wrong = None is the oracle (test_restated_layer_is_the_oracle)."""
    n, s, d = x.shape
    dk, b = d // 8, n * (s // ss)
    xb = x.reshape(b, ss, d)

    def heads(w):
        return (xb @ p[f"{prefix}multihead.{w}.weight"].t()).view(b, ss, 8, dk).transpose(1, 2)          # [b, 8, ss, dk]
    q, k, v = heads("Wq"), heads("Wk"), heads("Wv")
    i, j = torch.arange(ss)[:, None], torch.arange(ss)[None, :]
    scores = q @ k.transpose(2, 3)
    key = f"{prefix}multihead.Att.Krelpos"
    if key in p:
        m = (ss - 1 - (i - j) + (1 if wrong == "relpos+1" else 0)).clamp(0, ss - 1)
        scores = scores + (q @ p[key]).gather(3, m.expand(b, 8, ss, ss))
    keep = ((j < i) | ((i == 0) & (j == 0))) if wrong == "mask" else (j <= i)
    att = torch.softmax((scores / math.sqrt(dk)).masked_fill(~keep, float("-inf")), dim=3)
    ctx = (att @ v).transpose(1, 2).reshape(b, ss, d)
    y = O.layer_norm(xb + ctx @ p[f"{prefix}multihead.Wo.weight"].t(), p[f"{prefix}ln_multihead.weight"], p[f"{prefix}ln_multihead.bias"])
    ff = torch.relu(y @ p[f"{prefix}ffnetwork.lin1.weight"].t() + p[f"{prefix}ffnetwork.lin1.bias"])
    ff = ff @ p[f"{prefix}ffnetwork.lin2.weight"].t() + p[f"{prefix}ffnetwork.lin2.bias"]
    u = (y + ff) @ p[f"{prefix}last_linear.weight"].t() + p[f"{prefix}last_linear.bias"]
    width = d if wrong == "ln2" else u.shape[-1]
    mu = u.sum(-1, keepdim=True) / width
    var = ((u - mu) ** 2).sum(-1, keepdim=True) / width
    out = (u - mu) / torch.sqrt(var + 1e-5) * p[f"{prefix}ln_ffnetwork.weight"] + p[f"{prefix}ln_ffnetwork.bias"]
    return out.reshape(n, s, -1)


def run_torch(c, call, prob, wrong=None, accumulate=False, past_saved=False):
    """The call in plain float32 torch on the host: the f32 evaluation of the oracle (wrong = None), or layer_restated with one
    of its mistakes; accumulate: the gradients are added to what the buffers hold; past_saved: one word behind `saved` is written."""
    layer_fn = None if wrong is None else functools.partial(layer_restated, wrong=wrong)
    out, dx, grads = differentiate(prob.x, prob.p, prob.gout, c, prob.masks, torch.float32, check_margin=False, layer_fn=layer_fn)
    call.out.copy_(out)
    if c.dx:
        call.dx.copy_(dx)
    for l in range(c.layers):
        for i, name in enumerate(call.grad_names[l]):
            if name in prob.p:
                if accumulate:
                    call.grads[l][i] += grads[name]
                else:
                    call.grads[l][i].copy_(grads[name])
    call.saved.f32.zero_()
    call.scratch.f32.zero_()
    if past_saved:
        call.saved.all[GUARD + call.saved.words] = 0


RECTANGULAR, ODD = _case("B", 256, 40, 40, dout=64), _case("A", 64, 7, 21)
assert RECTANGULAR in CASES and ODD in CASES


def _host_call(c):
    prob = problem_of(c)
    return prob, Call(c, prob, 4096, 8192, "cpu")


@pytest.mark.parametrize("case", [RECTANGULAR, ODD, _case("C", 64, 32, 32, layers=2, nc=3, dx=False),
                                  _case("E", 128, 33, 66, p=P_DROP), _case("D", 64, 32, 64, wpack=False, gpack=False)], ids=_id)
def test_harness_accepts_the_f32_evaluation_of_the_oracle(case):
    prob, call = _host_call(case)
    with pytest.raises(AssertionError, match="not finite"):
        check_call(case, call, prob, book=False)                    # nothing written yet: NaN inside every window
    run_torch(case, call, prob)
    check_call(case, call, prob, book=False)


def test_restated_layer_is_the_oracle():
    for c in (RECTANGULAR, ODD):
        prob = problem_of(c)
        p64 = {k: v.double() for k, v in prob.p.items()}
        ref = oracle_forward(prob.x.double(), p64, c, prob.masks)
        assert rel_err(layer_restated(prob.x.double(), p64, _prefix(0), c.ss), ref) < 1e-13
        assert rel_err(ref, prob.out) == 0.0


@pytest.mark.parametrize("case,mistake", [(ODD, dict(wrong="relpos+1")), (RECTANGULAR, dict(wrong="relpos+1")), (ODD, dict(wrong="mask")),
                                          (RECTANGULAR, dict(wrong="mask")), (RECTANGULAR, dict(wrong="ln2")), (ODD, dict(accumulate=True)),
                                          (RECTANGULAR, dict(past_saved=True))],
                         ids=lambda v: _id(v) if isinstance(v, Case) else "-".join(f"{k}-{w}" for k, w in v.items()))
def test_harness_rejects_wrong_implementations(case, mistake):
    prob, call = _host_call(case)
    run_torch(case, call, prob, **mistake)
    with pytest.raises(AssertionError) as info:
        check_call(case, call, prob, book=False)
    expected = {"accumulate": "not finite", "past_saved": "outside the window of `saved`", "wrong": "rel err"}[next(iter(mistake))]
    assert expected in str(info.value), info.value


def test_harness_rejects_scratch_written_outside_its_window_by_the_forward_and_a_changed_input():
    prob, call = _host_call(ODD)
    run_torch(ODD, call, prob)
    call.scratch.all[GUARD - 1] = 0
    call.scratch_stray_after_forward = call.scratch.stray()
    call.scratch.poison()
    with pytest.raises(AssertionError, match="the forward wrote 1 words outside its scratch window, the first at word -1"):
        check_call(ODD, call, prob, book=False)
    prob, call = _host_call(ODD)
    run_torch(ODD, call, prob)
    call.x[0, 0, 0] += 1.0
    with pytest.raises(AssertionError, match="inputs were written"):
        check_call(ODD, call, prob, book=False)
