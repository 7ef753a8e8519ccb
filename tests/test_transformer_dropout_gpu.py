"""The transformer layer in TRAINING mode (dropout p = 0.1) against an exact fp64 oracle.

The kernels' dropout masks are a pure hash of (seed, element index) (csrc/common.h: drop_mul) and the seed is drawn from torch's
CPU generator (cpc2_amd/transformers.py), so oracle/dropmask.py rebuilds every mask bit for bit on the host and
O.transformer_layer_forward(drop=...) evaluates the layer in fp64 under exactly those masks: the output, dx and every parameter
gradient are then held to the eval-mode tolerances of tests/test_gpu_parity.py::test_transformer_vs_oracle_fp64 (2e-5 / 1e-4 /
2e-4; the criterion case to those of tests/test_criterion_pred_gpu.py).  Five pieces of device code have to agree on which
element is dropped -- the generic and the MFMA attention forward, their two backward kernels, the GEMM's staged-store epilogue
(and epi_pass_kernel in its place under cpc_gemm_set_mode(1)), the EPI_GATE adjoint that infers the mask from h > 0, and the
per-layer / feed-forward seeds -- and each case below is the smallest shape that reaches one of their paths.

Before comparing, the feed-forward net's ReLU decisions are put out of reach of fp32 rounding UNDER THE MASKS
(oracle/settle.py: attention dropout changes the pre-activations); every oracle run asserts that no fp64 pre-activation lies
within RELU_MARGIN of zero.  No element is excluded from any comparison.

Run with -s for the table of worst relative errors per case."""
import numpy as np
import pytest
import torch

import cpc2_amd
from cpc2_amd import _lib
from cpc2_amd.transformers import MultiClassifierTransformerHead, _TransformerFn, buildTransformerAR
from oracle import cpc_oracle as O
from oracle import dropmask as D
from oracle import synth
from oracle.mt19937 import MT19937, negative_indices
from oracle.settle import RELU_MARGIN, settle_relu_decisions

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = 0.1
TOL_OUT, TOL_DX, TOL_GRAD = 2e-5, 1e-4, 2e-4          # test_transformer_vs_oracle_fp64
PFX = "L0."

_WORST = {}         # case -> {"out" | "dx" | "grad": (worst relative error, where)}


def rel_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def assert_close(got, ref, tol, what="", rtol=None, book=None):
    """(tests/test_gpu_parity.py) max-norm check |got - ref|_inf <= tol * |ref|_inf AND, element by element,
    |got - ref| <= atol + rtol * |ref| with atol = tol * |ref|_inf and rtol = 64 * tol by default.  book = (case, quantity):
    where the error is kept for the module's report."""
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    e = rel_err(got, ref)
    if book is not None:
        slot = _WORST.setdefault(book[0], {})
        if e > slot.get(book[1], (-1.0, ""))[0]:
            slot[book[1]] = (e, what)
    assert e <= tol, f"{what}: rel err {e:.3e} > {tol:.1e}"
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    atol = tol * float(r.abs().max()) + 1e-30
    rt = 64 * tol if rtol is None else rtol
    bad = (g - r).abs() > atol + rt * r.abs()
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements outside atol {atol:.2e} + {rt:.1e} |ref|"


@pytest.fixture(scope="module", autouse=True)
def _report_worst_errors():
    yield
    print("\nworst relative errors of tests/test_transformer_dropout_gpu.py (tolerances: out %.0e, dx %.0e, grad %.0e):"
          % (TOL_OUT, TOL_DX, TOL_GRAD))
    for case in sorted(_WORST):
        print("  %-34s" % case + "  ".join(f"{q} {_WORST[case][q][0]:.3e} ({_WORST[case][q][1]})" for q in sorted(_WORST[case])))


def _sync():
    torch.cuda.synchronize()
    _lib.check(_lib.load().cpc_async_error_check(_lib.stream_ptr(torch.device(DEV))), "async errors")


# ----------------------------------------------------------------------------- building blocks
def _params(d_model, size_seq, seed, abspos=False, n_classifiers=1, prefix=PFX):
    p = synth.transformer_params(d_model, d_model, size_seq, seed, prefix=prefix, n_classifiers=n_classifiers)
    if abspos:
        del p[f"{prefix}multihead.Att.Krelpos"]
    return p


def _load(layer, p, prefix=PFX):
    sd = layer.state_dict()
    sd.update({k[len(prefix):]: v for k, v in p.items() if k.startswith(prefix)})
    layer.load_state_dict(sd)


def _abi_order(p, prefix):
    """The 15 tensors of a layer in the C ABI's order (TransformerLayer._param_list)."""
    names = ["multihead.Wq.weight", "multihead.Wk.weight", "multihead.Wv.weight", "multihead.Wo.weight", "multihead.Att.Krelpos",
             "ln_multihead.weight", "ln_multihead.bias", "ffnetwork.lin1.weight", "ffnetwork.lin1.bias", "ffnetwork.lin2.weight",
             "ffnetwork.lin2.bias", "last_linear.weight", "last_linear.bias", "ln_ffnetwork.weight", "ln_ffnetwork.bias"]
    return [prefix + n for n in names]


def _oracle_out(x_in, p64, layers, size_seq, n_classifiers=1, check_margin=True):
    """The stacked layers `layers` = [(prefix, drop)] in fp64 on x_in; n_classifiers belongs to the last one."""
    h = x_in
    for i, (prefix, drop) in enumerate(layers):
        pre = []
        h = O.transformer_layer_forward(h, p64, prefix, size_seq=size_seq, pre_out=pre, drop=drop,
                                        n_classifiers=n_classifiers if i == len(layers) - 1 else 1)
        if check_margin:
            assert float(pre[0].abs().min()) >= RELU_MARGIN, f"{prefix}: a ReLU decision within {RELU_MARGIN} of zero"
    return h


def _oracle(x, pe, p, layers, size_seq, gout, n_classifiers=1):
    """(out, dx, {name: gradient}) of sum(out * gout) in fp64 under the masks of `layers`."""
    p64 = {k: v.double().requires_grad_(True) for k, v in p.items()}
    x64 = x.double().requires_grad_(True)
    out = _oracle_out(x64 if pe is None else x64 + pe, p64, layers, size_seq, n_classifiers)
    (out * gout.double()).sum().backward()
    return out.detach(), x64.grad, {k: v.grad for k, v in p64.items()}


def _compare(case, got, ref):
    (out, dx, grads), (ref_out, ref_dx, ref_grads) = got, ref
    assert_close(out, ref_out, TOL_OUT, f"{case} out", book=(case, "out"))
    assert_close(dx, ref_dx, TOL_DX, f"{case} dx", book=(case, "dx"))
    assert set(grads) == set(ref_grads)
    for name in sorted(grads):
        assert grads[name] is not None, name
        assert_close(grads[name], ref_grads[name], TOL_GRAD, f"{case} grad {name}", book=(case, "grad"))


# ----------------------------------------------------------------------------- a-i, k: through the modules
#        d_model, size_seq, s, n, kind, torch.manual_seed
CASES = {
    "a-generic-dk8": (64, 32, 32, 2, "layer", 1),            # generic attention forward and backward, dk = 8
    "b-generic-chunks3": (64, 32, 96, 2, "layer", 2),        # chunks = 3: the chunk term of cid
    "c-generic-dk64-partial-tile": (512, 40, 40, 2, "layer", 3),     # generic kernels at dk = 64, partial query tile
    "d-mfma-full": (256, 128, 128, 2, "layer", 4),           # MFMA kernels, FULL
    "e-mfma-ragged": (256, 116, 116, 2, "layer", 5),         # MFMA, ragged last tile
    "f-mfma-chunks3-padded": (256, 32, 80, 3, "layer", 6),   # MFMA, chunks = 3, zero-padded tail: indices run over the padded tensor
    "g-ffn-32MB-nontemporal": (256, 128, 128, 32, "layer", 7),       # R = 4096: FFN activation = 32 MB, indices above 2^23
    "h-abspos": (64, 32, 32, 2, "abspos", 8),                # abspos=True through buildTransformerAR, no Krelpos
    "i-multi-classifier-head": (64, 32, 32, 2, "multi", 9),  # MultiClassifierTransformerHead, 3 classifiers
}
N_CLASSIFIERS = 3


def _build(case):
    """Everything of a case that does not touch the GPU: parameters (ReLU decisions settled under the masks), inputs, the
    module's seed and masks, the module itself (on the host)."""
    d_model, size_seq, s, n, kind, k = CASES[case]
    abspos, ncls = kind == "abspos", N_CLASSIFIERS if kind == "multi" else 1
    p = _params(d_model, size_seq, 400 + k, abspos=abspos, n_classifiers=ncls)
    x = synth.features((n, s, d_model), 420 + k, relu=True)
    gout = synth.features((n, s, d_model) if ncls == 1 else (n, s, ncls, d_model), 440 + k)
    if kind == "multi":
        net = layer = MultiClassifierTransformerHead(ncls, sizeSeq=size_seq, dmodel=d_model, dout=d_model)
    else:
        net = buildTransformerAR(d_model, d_model, 1, size_seq, abspos)
        layer = net[-1]
    # the position table as the module holds it (computed in fp32 by torch; "not on the measured path"): the oracle adds the same
    pe = net[0].pe[:, :s].double() if abspos else None
    torch.manual_seed(k)
    seed = D.draw_seed()
    masks = D.layer_masks(seed, n, s, size_seq, P)
    settle_relu_decisions(p, PFX, x.double() if pe is None else x.double() + pe, n_classifiers=ncls, size_seq=size_seq, drop=masks)
    _load(layer, p)
    return dict(p=p, x=x, gout=gout, net=net, layer=layer, pe=pe, seed=seed, masks=masks, size_seq=size_seq, ncls=ncls, k=k)


def _run_module(c):
    net, layer = c["net"].to(DEV).train(), c["layer"]
    xd = c["x"].to(DEV).requires_grad_(True)
    torch.manual_seed(c["k"])
    out = net(xd)
    (out * c["gout"].to(DEV)).sum().backward()
    _sync()
    return out.detach().cpu(), xd.grad.cpu(), {PFX + name: prm.grad.cpu() for name, prm in layer.named_parameters()}


SHARED = ("a-generic-dk8", "e-mfma-ragged")      # also the shapes of the negative controls: computed once, left unchanged
_RESULTS = {}


def _case(case):
    """(case data, the module's results, the oracle's)."""
    if case in _RESULTS:
        return _RESULTS[case]
    c = _build(case)
    got = _run_module(c)
    ref = _oracle(c["x"], c["pe"], c["p"], [(PFX, c["masks"])], c["size_seq"], c["gout"], c["ncls"])
    if case in SHARED:
        _RESULTS[case] = (c, got, ref)
    return c, got, ref


@pytest.mark.parametrize("case", list(CASES))
def test_training_mode_vs_oracle_fp64_under_the_rebuilt_masks(case):
    """The module in .train(): output, dx and every parameter gradient against the fp64 oracle under the masks rebuilt on the host
    from the seed the module drew."""
    c, got, ref = _case(case)
    d_model, size_seq, s, n = CASES[case][:4]
    chunks = -(-s // size_seq)
    assert c["masks"][0].shape == (n * 8 * chunks, size_seq, size_seq) and c["masks"][1].shape == (n * chunks * size_seq, 2048)
    if case.startswith("g"):
        assert c["masks"][1].numel() * 4 >= 32 << 20            # the GEMM's non-temporal store branch (gemm_f32.hip: vec_out = 2)
    _compare(case, got, ref)


def test_training_mode_under_the_f32_mfma_gemm_mode():
    """Case e under cpc_gemm_set_mode(1): the products are plain fp32 MFMA (K <= 2048) and the activation's ReLU + dropout runs
    as epi_pass_kernel instead of the staged-store epilogue -- the same masks, the same tolerances."""
    case = "e-mfma-ragged"
    c = _build(case)
    lib = _lib.load()
    prev = lib.cpc_gemm_set_mode(1)
    try:
        got = _run_module(c)
    finally:
        lib.cpc_gemm_set_mode(prev)
    ref = _oracle(c["x"], c["pe"], c["p"], [(PFX, c["masks"])], c["size_seq"], c["gout"])
    _compare("k-" + case[2:] + "-gemm-mode-1", got, ref)


# ----------------------------------------------------------------------------- j and the chosen seeds: _TransformerFn.apply
def _run_function(p, prefixes, x, gout, size_seq, seed):
    names = [n for prefix in prefixes for n in _abi_order(p, prefix)]
    tensors = [p[n].to(DEV).requires_grad_(True) for n in names]
    xd = x.to(DEV).requires_grad_(True)
    out = _TransformerFn.apply(xd, size_seq, len(prefixes), 1, P, seed, False, *tensors)
    (out * gout.to(DEV)).sum().backward()
    _sync()
    return out.detach().cpu(), xd.grad.cpu(), {n: t.grad.cpu() for n, t in zip(names, tensors)}


def test_two_stacked_layers_use_the_per_layer_seeds():
    """_TransformerFn.apply with n_layers = 2 on shape a: layer l runs under seed + 0x1000 * l (and its FFN under that ^ 0xFF)."""
    d_model, size_seq, s, n = 64, 32, 32, 2
    seed = 0x0123456789ABCDE
    prefixes = ["L0.", "L1."]
    p = {**_params(d_model, size_seq, 461, prefix="L0."), **_params(d_model, size_seq, 462, prefix="L1.")}
    x = synth.features((n, s, d_model), 463, relu=True)
    gout = synth.features((n, s, d_model), 464)
    layers = [(prefix, D.layer_masks(seed, n, s, size_seq, P, layer=l)) for l, prefix in enumerate(prefixes)]
    assert not torch.equal(layers[0][1][0], layers[1][1][0])
    settle_relu_decisions(p, "L0.", x, size_seq=size_seq, drop=layers[0][1])
    with torch.no_grad():
        h0 = O.transformer_layer_forward(x.double(), {k: v.double() for k, v in p.items()}, "L0.", size_seq=size_seq, drop=layers[0][1])
    settle_relu_decisions(p, "L1.", h0, size_seq=size_seq, drop=layers[1][1])
    got = _run_function(p, prefixes, x, gout, size_seq, seed)
    ref = _oracle(x, None, p, layers, size_seq, gout)
    _compare("j-two-layers", got, ref)


@pytest.mark.parametrize("seed", [0x12345678, 0x1234567800000000, 2 ** 62 - 1], ids=["high-word-zero", "low-word-zero", "2^62-1"])
def test_both_words_of_the_seed_reach_the_hash(seed):
    """_TransformerFn.apply on shape a with chosen 64-bit seeds: the high word zero, the low word zero, the largest the module
    can draw."""
    d_model, size_seq, s, n = 64, 32, 32, 2
    p = _params(d_model, size_seq, 471)
    x = synth.features((n, s, d_model), 472, relu=True)
    gout = synth.features((n, s, d_model), 473)
    masks = D.layer_masks(seed, n, s, size_seq, P)
    settle_relu_decisions(p, PFX, x, size_seq=size_seq, drop=masks)
    got = _run_function(p, [PFX], x, gout, size_seq, seed)
    ref = _oracle(x, None, p, [(PFX, masks)], size_seq, gout)
    _compare(f"seed-{seed:#x}", got, ref)


# ----------------------------------------------------------------------------- negative controls (oracle side only)
@pytest.mark.parametrize("case", SHARED)
def test_the_comparison_notices_a_wrong_mask(case):
    """The power of the comparison, pinned: the kernels' output is far (> 100 x the output tolerance) from the oracle under
    three WRONG sets of masks -- attention indices shifted by one, the FFN mask hashed under `seed` instead of seed ^ 0xFF, no
    masks at all.  (Measured on the oracle alone: such masks move its output by 0.11 - 0.17 of its scale.)  The kernels are
    never altered; a later change that makes the comparison vacuous fails here."""
    c, (out, _dx, _grads), (ref_out, _rdx, _rgrads) = _case(case)
    att, ffn = c["masks"]
    seed = c["seed"]
    wrong = {
        "attention index + 1": (torch.from_numpy(D.mask_values(seed, np.arange(att.numel(), dtype=np.uint64) + np.uint64(1), P)).view(att.shape), ffn),
        "ffn under seed, not seed ^ 0xFF": (att, torch.from_numpy(D.mask_values(seed, np.arange(ffn.numel(), dtype=np.uint64), P)).view(ffn.shape)),
        "no masks": None,
    }
    p64 = {k: v.double() for k, v in c["p"].items()}
    assert rel_err(out, ref_out) <= TOL_OUT
    for what, drop in wrong.items():
        with torch.no_grad():
            bad = _oracle_out(c["x"].double(), p64, [(PFX, drop)], c["size_seq"], check_margin=False)
        e = rel_err(out, bad)
        print(f"\n  negative control {case}, {what}: rel err {e:.3e}")
        assert e > 100 * TOL_OUT, f"{case}, {what}: rel err {e:.3e} does not stand out"


# ----------------------------------------------------------------------------- the seed stream
def test_consecutive_calls_draw_consecutive_seeds_and_eval_draws_none():
    """Two training-mode calls after one torch.manual_seed use the first and the second draw_seed() value (each output against
    the oracle under ITS masks); an eval() call leaves torch's generator where it was."""
    d_model, size_seq, s, n = 64, 32, 32, 2
    p = _params(d_model, size_seq, 481)
    x = synth.features((n, s, d_model), 482, relu=True)
    torch.manual_seed(21)
    seeds = [D.draw_seed(), D.draw_seed()]
    assert seeds[0] != seeds[1]
    masks = [D.layer_masks(sd, n, s, size_seq, P) for sd in seeds]
    for _ in range(4):                  # (a bias raised for one set of masks may bring a unit near zero under the other)
        for m in masks:
            settle_relu_decisions(p, PFX, x, size_seq=size_seq, drop=m)
    net = buildTransformerAR(d_model, d_model, 1, size_seq, False)
    _load(net[0], p)
    net = net.to(DEV).train()
    xd = x.to(DEV)
    torch.manual_seed(21)
    with torch.no_grad():
        outs = [net(xd), net(xd)]
        state = torch.get_rng_state()
        net.eval()
        plain = net(xd)
        assert torch.equal(torch.get_rng_state(), state)
    _sync()
    assert D.draw_seed() not in seeds                     # (the stream stands behind the two draws)
    p64 = {k: v.double() for k, v in p.items()}
    for i in range(2):
        ref = _oracle_out(x.double(), p64, [(PFX, masks[i])], size_seq)
        assert_close(outs[i].cpu(), ref, TOL_OUT, f"call {i}", book=("seed-stream", f"out{i}"))
    assert_close(plain.cpu(), _oracle_out(x.double(), p64, [(PFX, None)], size_seq, check_margin=False), TOL_OUT, "eval call")
    assert rel_err(outs[0], outs[1]) > 100 * TOL_OUT


# ----------------------------------------------------------------------------- the criterion's predictors
def test_criterion_transformer_predictors_in_training_mode_vs_oracle_fp64():
    """CPCUnsupersivedCriterion(..., rnnMode='transformer') in .train() at the smallest shape tests/test_criterion_pred_gpu.py
    runs that mode at (Har = Henc = 256, T 128, K 12, 128 negatives, b = 3; the predictors see c[:, :116], sizeSeq 116): the
    losses, dc, dz (and the predictors' gradients) against O.criterion_forward with every predictor under its own masks, at
    that file's tolerances for the eval-mode case (1e-5 / 2e-4 / 1e-4 / 5e-4).

    Order of the draws from torch's CPU generator in CPCUnsupersivedCriterion.forward (cpc2_amd/criterion.py): first
    sampleIndices -- the NegativeSampler consumes torch's generator for the negative indices UNLESS the criterion was given a
    private index stream with crit.seed(), as here and in every test of that file -- then _predictions, which calls the K
    predictors in ModuleList order, each TransformerLayer.forward drawing ONE seed (cpc2_amd/transformers.py).  The criterion's
    own nn.Dropout(0.5) (dropout=True only; off here) draws from the device's generator, not the CPU's.  So after
    torch.manual_seed(s) the K seeds are K consecutive draw_seed() values."""
    h, nn, b, t_len, k, idx_seed, drop_seed = 256, 128, 3, 128, 12, 811, 31
    w_len = t_len - k
    c = synth.features((b, t_len, h), 801)
    z = synth.features((b, t_len, h), 802, relu=True)
    p = {}
    for i in range(k):
        p.update(synth.transformer_params(h, h, w_len, seed=820 + i, prefix=f"wPrediction.predictors.{i}.0."))
    torch.manual_seed(drop_seed)
    seeds = [D.draw_seed() for _ in range(k)]
    masks = [D.layer_masks(sd, b, w_len, w_len, P) for sd in seeds]
    for i in range(k):
        settle_relu_decisions(p, f"wPrediction.predictors.{i}.0.", c[:, :w_len], drop=masks[i])
    crit = cpc2_amd.CPCUnsupersivedCriterion(k, h, h, nn, rnnMode="transformer", sizeInputSeq=t_len)
    sd = crit.state_dict()
    assert set(p) <= set(sd) and {n for n, _ in crit.named_parameters()} == set(p)
    sd.update(p)
    crit.load_state_dict(sd)
    crit = crit.to(DEV).train()
    cd, zd = c.to(DEV).requires_grad_(True), z.to(DEV).requires_grad_(True)
    crit.seed(idx_seed)
    torch.manual_seed(drop_seed)
    losses, acc = crit(cd, zd, None)
    losses.sum().backward()
    _sync()
    assert D.draw_seed() not in seeds and torch.initial_seed() == drop_seed

    p64 = {n: v.double().requires_grad_(True) for n, v in p.items()}
    c64, z64 = c.double().requires_grad_(True), z.double().requires_grad_(True)
    _, _, ext = negative_indices(MT19937(idx_seed), b, t_len, w_len, nn)

    def predictor(i):
        def run(cw):
            pre = []
            out = O.transformer_layer_forward(cw, p64, f"wPrediction.predictors.{i}.0.", pre_out=pre, drop=masks[i])
            assert float(pre[0].abs().min()) >= RELU_MARGIN
            return out
        return run
    ref_losses, ref_acc = O.criterion_forward(c64, z64, [predictor(i) for i in range(k)], ext, nn)
    ref_losses.sum().backward()
    case = "criterion-transformer-predictors"
    assert losses.shape == ref_losses.shape
    assert_close(losses, ref_losses, 1e-5, "criterion losses", book=(case, "losses"))
    assert torch.allclose(acc.cpu().double(), ref_acc, atol=2.5 / (b * w_len))
    assert_close(cd.grad, c64.grad, 2e-4, "criterion dc", book=(case, "dc"))
    assert_close(zd.grad, z64.grad, 1e-4, "criterion dz", book=(case, "dz"))
    for name, prm in crit.named_parameters():
        assert_close(prm.grad, p64[name].grad, 5e-4, f"criterion grad {name}", book=(case, "grad"))
