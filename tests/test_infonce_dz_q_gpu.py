"""The criterion's dz with LINEAR predictors through per-row context sums (csrc/infonce.hip: infonce_bwd_fused_kernel<.., false>,
infonce_dz_q_kernel, dz = Q . wq^T; chosen with CPC_NCE_DZ=q) against the contribution-row path (CPC_NCE_DZ=rows and the default:
also the module predictors' path).  Every case runs the SAME inputs through both paths: dc, dP and dW_k are bit-identical (their
kernels' arithmetic has not changed), dz is held to the fp64 oracle within TWICE the contribution-row path's own maximum element
error on those inputs (the factor covers the extra rounding of the final product; the summation length is the same), z rows nobody
refers to are exactly zero, and two launches give the same dz bit for bit.  H = 256 (once 512), K = 12.  The helpers, with a guard
of 4096 bytes behind `saved` and `scratch` that no launch may touch, are in tests/infonce_dz_harness.py; the rest of the path's domain
is in tests/test_infonce_dz_q_domain_gpu.py."""
import pytest
import torch

import cpc2_amd
from cpc2_amd.train import buildOptimizer, cpcStep
from oracle import cpc_oracle as O
from oracle import synth
from tests.infonce_dz_harness import DEV, _check, _random_ext

pytestmark = pytest.mark.gpu
K = 12


def test_small_base_case(monkeypatch):
    """b = 3, T = 20 (W = 8), 16 negatives.  Measured maximum element error of dz against the fp64 oracle: contribution rows
    6.02e-10, per-row sums 1.02e-09 (largest |dz| 2.07e-03)."""
    _check(monkeypatch, 3, 20, 256, 16, _random_ext(3, 20, 16, 11), seed=500)


def test_duplicate_negatives_and_a_row_drawn_by_many(monkeypatch):
    """The same, with one (b,t) whose negatives hold the same row twice (and three times), and one row drawn by every (b,t).
    Measured: contribution rows 9.64e-10, per-row sums 8.96e-10 (largest |dz| 2.13e-03)."""
    b, t_len, nn = 3, 20, 16
    ext = _random_ext(b, t_len, nn, 12).reshape(b, nn, t_len - K)
    ext[1, 3, 2] = ext[1, 9, 2] = 27                  # (b, t) = (1, 2): row 27 twice ...
    ext[2, 0, 5] = ext[2, 1, 5] = ext[2, 15, 5] = 4   # ... (2, 5): row 4 three times
    ext[:, 7, :] = 41                                 # row 41: negative 7 of every (b, t)
    _check(monkeypatch, b, t_len, 256, nn, ext, seed=510)


def test_block_boundaries_and_a_dead_row(monkeypatch):
    """b = 2, T = 140 (W = 128, a multiple of every tile), 128 negatives drawn from the rows that are no multiple of 3: the z rows
    span many blocks of the list sort, and frame 0 of window 0 (row 0) has no reference at all.
    Measured: contribution rows 1.01e-10, per-row sums 1.31e-10 (largest |dz| 2.82e-04)."""
    b, t_len, nn = 2, 140, 128
    rows = [r for r in range(b * t_len) if r % 3 != 0]
    dead = _check(monkeypatch, b, t_len, 256, nn, _random_ext(b, t_len, nn, 13, rows), seed=520)
    assert dead >= 1


def test_sample_weights(monkeypatch):
    """The b = 3 case with signal_quality given: one weight per window, the last window's the floor 1e-5 (criterion.py:230).
    Measured: contribution rows 4.81e-10, per-row sums 8.71e-10 (largest |dz| 1.34e-03)."""
    b, t_len = 3, 20
    q = torch.rand(b, 9, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    q[b - 1] = -1000.0
    weights = O.quality_weights(q, 2.0, 0.1, t_len - K)
    assert float(weights.min()) == 1e-5 and float(weights.max()) > 0.5
    _check(monkeypatch, b, t_len, 256, 16, _random_ext(b, t_len, 16, 14), seed=530, weights=weights)


def test_width_512(monkeypatch):
    """H = 512 (four waves per z row in the sum kernel, four per (b,t) in the backward kernel): b = 2, T = 20, 16 negatives.
    Measured: contribution rows 6.62e-10, per-row sums 7.31e-10 (largest |dz| 1.86e-03)."""
    _check(monkeypatch, 2, 20, 512, 16, _random_ext(2, 20, 16, 15), seed=540)


def test_deferred_form_through_cpcstep(monkeypatch):
    """b = 3 windows of 20 frames through cpcStep, 16 negatives, conventions of test_deferred_criterion_backward_gives_the_same_step_
    bit_for_bit: with the per-row sums, the deferred form (Q, the product and dW on the side stream beside the recurrent backward,
    joined where the encoder output's gradient is summed) gives every gradient of the immediate form bit for bit.  Between the two dz
    paths, the gradients that do not pass through dz -- the predictors' (dW) and the context network's (from dc) -- are equal bit for
    bit, and the encoder's, two f32 roundings of the same sums, agree to 1e-4 of the largest (the suite's bar for dz)."""
    from cpc2_amd import _route as route_mod
    hidden, b = 256, 3
    out = {}
    for mode, defer in (("q", True), ("q", False), ("rows", True)):
        monkeypatch.setenv("CPC_NCE_DZ", mode)
        if defer:
            monkeypatch.delenv("CPC_NCE_NO_DEFER", raising=False)
        else:
            monkeypatch.setenv("CPC_NCE_NO_DEFER", "1")
        mp = synth.encoder_params(hidden, 21)
        mp.update(synth.gru_params(hidden, hidden, 1, 22))
        model = cpc2_amd.CPCModel(cpc2_amd.CPCEncoder(hidden), cpc2_amd.CPCAR(hidden, hidden, False, 1))
        model.load_state_dict(mp)
        crit = cpc2_amd.CPCUnsupersivedCriterion(K, hidden, hidden, 16, rnnMode="linear", sizeInputSeq=20)
        crit.load_state_dict(synth.predictor_params(K, hidden, hidden, 23))
        model, crit = model.to(DEV), crit.to(DEV)
        opt = buildOptimizer(model, crit, lr=2e-4)
        crit.seed(5)
        x = synth.audio_windows(b, 20 * 160, 24).to(DEV)
        tot, _losses, _acc = cpcStep(x, x, torch.zeros(b, dtype=torch.long, device=DEV), model, crit)
        tot.backward()
        assert not route_mod._deferred, "a deferred backward is still pending after the backward pass"
        torch.cuda.synchronize()
        named = list(model.named_parameters()) + [("crit." + n, p) for n, p in crit.named_parameters()]
        out[(mode, defer)] = {n: opt.flat_grad[p._cpc_flat[1]:p._cpc_flat[1] + p.numel()].detach().clone() for n, p in named}
    q_def, q_imm, rows_def = out[("q", True)], out[("q", False)], out[("rows", True)]
    for n in q_def:
        assert torch.equal(q_def[n], q_imm[n]), f"{n}: deferred and immediate forms differ"
        assert float(q_def[n].abs().max()) > 0, n
        if n.startswith("gEncoder."):
            err = float((q_def[n].double() - rows_def[n].double()).abs().max())
            assert err <= 1e-4 * float(rows_def[n].abs().max()), f"{n}: {err:.3e}"
        else:
            assert torch.equal(q_def[n], rows_def[n]), f"{n} differs between the two dz paths"
