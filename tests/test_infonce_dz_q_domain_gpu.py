"""The criterion's dz through per-row context sums (CPC_NCE_DZ=q: infonce_bwd_fused_kernel<H, NKK, false>, infonce_dz_q_kernel<256|512>,
nce_wq_kernel, dz = Q . wq^T) across the domain nce_dz_q_wanted accepts, and the fallback just outside it.  tests/test_infonce_dz_q_gpu.py
holds the path at K = 12, Har = Henc, T context frames; here: every K class, Har != Henc, the candidate and staging limits,
c_frames = W, odd z-row counts, W = 1, reference lists of every length class of the sum kernel's 64-entry chunks and 8-entry groups
(and one beyond NCE_SORT_MAX), loss gradients with a zero and a negative entry, a window at the floor weight.

Every case goes through the C entries once with `rows` and twice with `q` on the same inputs (tests/infonce_dz_harness.py: _check):
dc, dP, dW_k and the losses bit-identical between the paths; dz of two `q` launches bit-identical; unreferred z rows exactly zero on
both; the guard bytes behind `saved` and `scratch` untouched; the linear entries' scratch need differs between the modes (the
evidence that the sums ran); losses, dc, dz and dW of BOTH paths within 1e-5 / 1e-4 / 1e-4 / 2e-4 of the largest element of the fp64
oracle's (the bounds test_criterion_odd_shapes_vs_oracle_fp64 holds the default path to); and the sums' maximum element error of dz
at most FACTOR x the contribution rows' own on those inputs -- 2.0 as in the K = 12 file wherever the measured ratio was at most 1.5,
twice the measured ratio elsewhere (never above 8), with the floor 2^-22 max|dz| where the rows path's error is next to nothing (K = 1,
W = 1: a contribution row is then a single product, and the ratio says nothing).  Outside the domain every output, dz included, is
bit-identical and the scratch need is equal.  tests/test_infonce_dz_q_domain_cpu.py holds the table and the constructed lists to
what is claimed of them here."""
import pytest
import torch

import cpc2_amd
from cpc2_amd import _lib
from cpc2_amd.criterion import _InfoNCEPredFn
from oracle import cpc_oracle as O
from oracle import synth
from oracle.mt19937 import MT19937, negative_indices
from tests import infonce_dz_harness as H

pytestmark = pytest.mark.gpu
DEV = H.DEV

# case -> factor of the tight gate where the measured ratio exceeds 1.5: twice that ratio (the measurements are in the docstrings;
# both paths sum in a fixed order, so the figures repeat from run to run).  No ratio is above 4.
FACTOR = {"steps-K1-h256": 3.34, "steps-K4-h256": 4.48, "steps-K5-h256": 4.82, "steps-K8-h256": 3.10, "steps-K9-h256": 3.48,
          "one-frame": 3.10, "widths-256-512-K16": 3.10, "corner-h256-K16-n128": 3.48, "cw-base": 3.38, "cw-widths-256-512": 3.16,
          "dlosses": 3.34, "floor-weight-K5": 4.94}


def _run(monkeypatch, cs, ext=None, **kw):
    ext = H._random_ext(cs.b, cs.t, cs.nn, cs.seed + 7, k=cs.k) if ext is None else ext
    kw.setdefault("factor", FACTOR.get(cs.name, 2.0))
    return H._check(monkeypatch, cs.b, cs.t, cs.har, cs.nn, ext, seed=cs.seed, k=cs.k, henc=cs.henc,
                    c_frames=cs.t - cs.k if cs.c_w else None, floor=cs.floor, structural=True, tag=cs.name, **kw)


@pytest.mark.parametrize("case", [cs for cs in H.CASES if cs.inside], ids=lambda cs: cs.name)
def test_domain_case_vs_rows_path_and_oracle_fp64(case, monkeypatch):
    """Inside the domain.  Measured maximum element error of dz against the fp64 oracle: contribution rows, per-row sums, their
    ratio, largest |dz| (and the factor where it is not 2.0):
      steps-K1-h256          1.313e-10  2.192e-10  1.67  3.690e-04   factor 3.34
      steps-K4-h256          5.227e-10  1.173e-09  2.24  1.344e-03   factor 4.48
      steps-K5-h256          5.521e-10  1.332e-09  2.41  1.824e-03   factor 4.82
      steps-K8-h256          5.680e-10  8.788e-10  1.55  1.873e-03   factor 3.10
      steps-K9-h256          5.859e-10  1.018e-09  1.74  1.935e-03   factor 3.48
      steps-K13-h256         8.260e-10  1.225e-09  1.48  2.024e-03
      steps-K16-h256         9.410e-10  1.293e-09  1.37  2.356e-03
      steps-K1-h512          1.274e-10  1.120e-10  0.88  1.737e-04
      steps-K13-h512         5.046e-10  4.945e-10  0.98  1.136e-03
      steps-K16-h512         5.132e-10  4.670e-10  0.91  1.377e-03
      one-frame              7.048e-09  1.090e-08  1.55  1.888e-02   factor 3.10
      widths-256-512-K12     5.662e-10  7.249e-10  1.28  1.908e-03
      widths-256-512-K16     5.281e-10  8.159e-10  1.55  1.687e-03   factor 3.10
      widths-512-256-K12     1.429e-09  1.281e-09  0.90  3.076e-03
      widths-512-256-K16     1.409e-09  1.302e-09  0.92  3.504e-03
      corner-h256-K16-n128   9.119e-10  1.591e-09  1.74  4.206e-03   factor 3.48
      corner-h256-K12-n176   1.072e-09  1.492e-09  1.39  3.026e-03
      corner-h256-K8-n256    9.783e-10  1.371e-09  1.40  2.573e-03
      corner-h512-K16-n256   7.822e-10  8.363e-10  1.07  2.159e-03
      corner-h512-K15-n272   8.946e-10  8.491e-10  0.95  1.640e-03
      cw-base                6.445e-10  1.091e-09  1.69  2.101e-03   factor 3.38
      cw-widths-256-512      5.457e-10  8.616e-10  1.58  1.665e-03   factor 3.16
    The ratio is largest where a contribution row has few terms (K = 4, 5: the rows path's own error is then smallest) and the context
    is 256 wide; every error is within 4 x 2^-22 of the largest |dz|."""
    assert H.q_domain(case.b, case.t, case.k, case.har, case.henc, case.nn)
    _run(monkeypatch, case)


@pytest.mark.parametrize("case", [cs for cs in H.CASES if not cs.inside], ids=lambda cs: cs.name)
def test_just_outside_the_domain_q_is_the_rows_path(case, monkeypatch):
    """The fallback contract: a shape nce_dz_q_wanted refuses (staging limit, Nneg % 16, lw > 320, Har or Henc 128) gives under
    CPC_NCE_DZ=q every output of CPC_NCE_DZ=rows bit for bit, dz included, with the same scratch need (asserted in _backward)."""
    assert not H.q_domain(case.b, case.t, case.k, case.har, case.henc, case.nn)
    _run(monkeypatch, case)


def test_one_target_frame_with_a_dead_row(monkeypatch):
    """W = 1 (b = 1, T = 13): every negative of the single (b,t) out of frames 1 .. 12, so that frame 0 has no reference; every
    later frame is the positive of exactly one step.  Measured: contribution rows 7.814e-09, per-row sums 8.948e-09, ratio 1.15 (largest |dz|
    1.980e-02)."""
    cs = H.CASE_BY_NAME["one-frame"]
    dead = _run(monkeypatch, cs, ext=H._random_ext(cs.b, cs.t, cs.nn, cs.seed, rows=range(1, cs.t), k=cs.k), factor=2.0)
    assert dead == 1


def test_reference_list_lengths(monkeypatch):
    """b = 2, T = 140, K = 12, 16 negatives: 4096 references over 280 rows, constructed (H.lists_ext) so that named rows receive
    exactly 0, 1, 7, 8, 9, 63, 64, 65, 128 and 600 of them -- around the 8-entry groups and the 64-entry chunks of the sum kernel,
    and one list beyond NCE_SORT_MAX, which stays unsorted: the bit-reproducibility assertion leaves out that row alone (_check
    asserts that it is exactly one); against the oracle it is held like every other row.  One row has positives only, frame 0 of
    window 0 negatives only, frame 0 of window 1 nothing.  Measured, two runs (the 600-entry list is summed in
    another order on BOTH paths): contribution rows 5.502e-10 / 4.121e-10, per-row sums 2.958e-10 / 3.867e-10, ratio 0.54 / 0.94 (largest
    |dz| 6.781e-04)."""
    cs = H.LISTS
    dead = _run(monkeypatch, cs, ext=H.lists_ext(), unsorted=1)
    assert dead == 1


def test_loss_gradients_with_a_zero_and_a_negative_entry(monkeypatch):
    """dlosses[3] = 0, dlosses[7] = -0.75 at the base shape: the zeroed step's coefficients are zeros, so its dW is exactly zero
    on both paths and dz (held to the oracle with the same dlosses) is what the other eleven steps give.
    Measured: contribution rows 6.403e-10, per-row sums 1.072e-09, ratio 1.67 (largest |dz| 2.267e-03): factor 3.34."""
    cs = H.DLOSSES
    dl = H.default_dlosses(cs.k)
    dl[3], dl[7] = 0.0, -0.75
    ext = H._random_ext(cs.b, cs.t, cs.nn, cs.seed, k=cs.k)
    _run(monkeypatch, cs, ext=ext, dlosses=dl)
    c, z, wk = H._inputs(cs.b, cs.t, cs.har, cs.seed, k=cs.k)
    for mode in ("rows", "q"):
        dw = H._backward(mode, monkeypatch, c, z, wk, ext, cs.nn, None, dlosses=dl)[0][2]
        assert float(dw[3].abs().max()) == 0.0 and float(dw[7].abs().max()) > 0, mode


def test_floor_weight_window_at_five_steps(monkeypatch):
    """K = 5 (b = 3, T = 13) with signal-quality weights, the last window's the floor 1e-5 (criterion.py:230).
    Measured: contribution rows 3.080e-10, per-row sums 7.605e-10, ratio 2.47 (largest |dz| 1.088e-03): factor 4.94."""
    cs = H.FLOOR_WEIGHT
    q = torch.rand(cs.b, 9, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    q[cs.b - 1] = -1000.0
    weights = O.quality_weights(q, 2.0, 0.1, cs.t - cs.k)
    assert float(weights.min()) == 1e-5 and float(weights.max()) > 0.5
    _run(monkeypatch, cs, weights=weights)


def test_module_predictor_entries_ignore_the_switch(monkeypatch):
    """cpc_infonce_forward_pred / cpc_infonce_backward_pred at H = 256, K = 12, 16 negatives under CPC_NCE_DZ=q and =rows: losses,
    accuracies, dz and the K dP bit-identical (these entries keep the contribution rows), and the scratch need for every entry
    (dim_ar > 0) under `q` covers the linear entries' need of both modes."""
    cs = H.PRED
    lib = _lib.load()
    w_len = cs.t - cs.k
    z = synth.features((cs.b, cs.t, cs.henc), cs.seed, relu=True)
    preds = [synth.features((cs.b, w_len, cs.henc), cs.seed + 1 + i, scale=2.0) for i in range(cs.k)]
    ext_raw = H._random_ext(cs.b, cs.t, cs.nn, cs.seed, k=cs.k)
    ext = H._time_major(ext_raw, cs.b, w_len, cs.nn).to(DEV)
    g = H.default_dlosses(cs.k).to(DEV)
    outs, need = {}, {}
    for mode in ("rows", "q"):
        monkeypatch.setenv("CPC_NCE_DZ", mode)
        need[mode] = lib.cpc_infonce_scratch_bytes(cs.b, cs.t, cs.k, -cs.har, cs.henc, cs.nn)
        need[mode, "all"] = lib.cpc_infonce_scratch_bytes(cs.b, cs.t, cs.k, cs.har, cs.henc, cs.nn)
        zd = z.to(DEV).requires_grad_(True)
        pd = [p.to(DEV).requires_grad_(True) for p in preds]
        losses, acc = _InfoNCEPredFn.apply(zd, ext, None, cs.nn, *pd)
        (losses * g).sum().backward()
        torch.cuda.synchronize()
        _lib.check(lib.cpc_async_error_check(_lib.stream_ptr(zd.device)), "async errors")
        outs[mode] = [losses.detach(), acc.detach(), zd.grad] + [p.grad for p in pd]
    assert need["q"] != need["rows"] and need["q", "all"] >= max(need["q"], need["rows"]) and need["rows", "all"] == need["rows"]
    for i, (a, bb) in enumerate(zip(outs["rows"], outs["q"])):
        assert torch.equal(a, bb), f"output {i} of the module-predictor entries depends on CPC_NCE_DZ"
    ref = O.criterion_forward_sparse(None, z.double(), [p.double() for p in preds], ext_raw.reshape(-1), cs.nn,
                                     dlosses=H.default_dlosses(cs.k, torch.float64))
    err = float((outs["q"][2].cpu().double() - ref["dz"]).abs().max())
    assert err <= 1e-4 * float(ref["dz"].abs().max())


@pytest.mark.parametrize("variant", ["plain", "skip", "reverse", "quality"])
def test_criterion_module_under_q_vs_oracle_fp64(variant, monkeypatch):
    """CPCUnsupersivedCriterion with rnnMode='linear' at Har = Henc = 256 (b = 3, T = 40, K = 12, 32 negatives) under CPC_NCE_DZ=q,
    with n_skipped = 2, mode='reverse' and the signal-quality weights, against O.criterion_forward exactly as
    test_criterion_variants_at_hidden_256_512_vs_oracle_fp64 does (whose Har = 64 never reaches the sum kernels)."""
    cs = H.MODULE
    b, t_len, har, henc, k, nn = cs.b, cs.t, cs.har, cs.henc, cs.k, cs.nn
    monkeypatch.setenv("CPC_NCE_DZ", "rows")
    rows_need = _lib.load().cpc_infonce_scratch_bytes(b, t_len, k, -har, henc, nn)
    monkeypatch.setenv("CPC_NCE_DZ", "q")
    assert _lib.load().cpc_infonce_scratch_bytes(b, t_len, k, -har, henc, nn) != rows_need
    kw, okw = {}, {}
    if variant == "skip":
        kw["n_skipped"] = okw["n_skipped"] = 2
    if variant == "reverse":
        kw["mode"] = okw["mode"] = "reverse"
    if variant == "quality":
        kw.update(growth_rate=2.0, inflection_point_x=0.1)
    crit = cpc2_amd.CPCUnsupersivedCriterion(k, har, henc, nn, rnnMode="linear", sizeInputSeq=999, **kw)
    cp = synth.predictor_params(k, har, henc, seed=cs.seed, scale=3.0)
    crit.load_state_dict(cp)
    crit = crit.to(DEV)
    c = synth.features((b, t_len, har), cs.seed + 1)
    z = synth.features((b, t_len, henc), cs.seed + 2, relu=True)
    quality = torch.rand(b, 9, generator=torch.Generator().manual_seed(5)) if variant == "quality" else None
    if quality is not None:
        okw["weights"] = O.quality_weights(quality.double(), 2.0, 0.1, t_len - k)
    cd, zd = c.to(DEV).requires_grad_(True), z.to(DEV).requires_grad_(True)
    crit.seed(78)
    losses, acc = crit(cd, zd, None, None if quality is None else quality.to(DEV))
    losses.sum().backward()
    torch.cuda.synchronize()
    p64 = {n: v.double().requires_grad_(True) for n, v in cp.items()}
    c64, z64 = c.double().requires_grad_(True), z.double().requires_grad_(True)
    _, _, ext = negative_indices(MT19937(78), b, t_len, t_len - k, nn)
    ref_losses, ref_acc = O.criterion_forward(c64, z64, O.predictor_list(p64, k), ext, nn, **okw)
    ref_losses.sum().backward()

    def close(got, ref, tol, what):
        err = float((got.detach().double().cpu() - ref).abs().max())
        assert err <= tol * float(ref.abs().max()), f"{what}: {err:.3e} (largest {float(ref.abs().max()):.3e})"

    assert losses.shape == ref_losses.shape
    close(losses, ref_losses.detach(), 1e-5, "losses")
    assert torch.allclose(acc.cpu().double(), ref_acc, atol=2.5 / (b * (t_len - k)))
    close(cd.grad, c64.grad, 1e-4, "dc")
    close(zd.grad, z64.grad, 1e-4, "dz")
    for i in range(k):
        ref = p64[f"wPrediction.predictors.{i}.weight"].grad
        got = crit.wPrediction.predictors[i].weight.grad
        if ref is None or float(ref.abs().max()) == 0.0:
            assert got is None or float(got.abs().max()) == 0.0
        else:
            close(got, ref, 2e-4, f"dW{i}")
