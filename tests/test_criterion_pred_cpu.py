"""oracle.criterion_forward_sparse with PRECOMPUTED predictions (the checker of the module-predictor kernels at b = 64,
tests/test_criterion_pred_gpu.py) against the dense autograd restatement with the same predictions handed over as callables,
in float64; the linear form's return value is pinned by tests/test_oracle_golden.py and stays as it was."""
import numpy as np
import pytest
import torch

from oracle import cpc_oracle as O
from oracle import synth
from oracle.mt19937 import MT19937, negative_indices


def _close(got, ref, what, tol=1e-12):
    err = float((got.double() - ref.double()).abs().max() / (ref.double().abs().max() + 1e-300))
    assert err <= tol, f"{what}: {err:.2e}"


@pytest.mark.parametrize("tag", ["plain", "skip", "reverse", "quality", "skip_reverse_quality", "one_frame", "many_negatives"])
def test_sparse_criterion_with_predictions_is_the_dense_one(tag):
    b, t_len, henc, k, nn, seed = 5, 32, 32, 4, 16, 11
    okw = {}
    if "skip" in tag:
        okw["n_skipped"] = 1
    if "reverse" in tag:
        okw["mode"] = "reverse"
    if tag == "one_frame":
        t_len = k + 1
    if tag == "many_negatives":
        b, t_len, henc, k, nn = 3, 33, 128, 7, 129
    w_len = t_len - k
    if "quality" in tag:
        quality = torch.rand(b, 9, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
        quality[1] = -1000.0                                   # (the weight of window 1 is the floor 1e-5)
        okw["weights"] = O.quality_weights(quality, 2.0, 0.1, w_len)
        assert float(okw["weights"].min()) == 1e-5
    preds = [synth.features((b, w_len, henc), 40 + i, scale=2.0).double().requires_grad_(True) for i in range(k)]
    z = synth.features((b, t_len, henc), 39, relu=True).double().requires_grad_(True)
    _, _, ext = negative_indices(MT19937(seed), b, t_len, w_len, nn)
    dummy_c = torch.zeros(b, t_len, 1, dtype=torch.float64)
    losses, acc = O.criterion_forward(dummy_c, z, [(lambda c, p=p: p) for p in preds], ext, nn, **okw)
    dl = torch.linspace(0.5, 1.5, losses.shape[1], dtype=torch.float64)
    (losses * dl).sum().backward()
    got = O.criterion_forward_sparse(None, z, [p.detach() for p in preds], ext, nn, dlosses=dl, windows_per_chunk=2, **okw)
    assert sorted(got) == ["acc", "dP", "dz", "losses"]
    _close(got["losses"], losses.detach(), "losses")
    _close(got["acc"], acc, "acc")
    _close(got["dz"], z.grad, "dz")
    assert len(got["dP"]) == k
    for i, p in enumerate(preds):
        if p.grad is None or float(p.grad.abs().max()) == 0.0:
            assert float(got["dP"][i].abs().max()) == 0.0, f"dP{i} of a skipped step"
        else:
            _close(got["dP"][i], p.grad, f"dP{i}")


def test_sparse_criterion_linear_form_is_unchanged():
    """Matrices in: the same keys as ever, and the same numbers as the prediction form fed with c W_k^T."""
    b, t_len, har, henc, k, nn = 3, 20, 24, 32, 4, 8
    p = synth.predictor_params(k, har, henc, seed=3, scale=3.0)
    wk = [p[f"wPrediction.predictors.{i}.weight"].double() for i in range(k)]
    c = synth.features((b, t_len, har), 4).double()
    z = synth.features((b, t_len, henc), 5, relu=True).double()
    _, _, ext = negative_indices(MT19937(2), b, t_len, t_len - k, nn)
    lin = O.criterion_forward_sparse(c, z, wk, ext, nn, mode="reverse")
    assert sorted(lin) == ["acc", "dW", "dc", "dz", "losses"]
    cw = torch.flip(c, [1])[:, :t_len - k]
    given = O.criterion_forward_sparse(None, z, [cw @ w.t() for w in wk], ext, nn, mode="reverse")
    _close(given["losses"], lin["losses"], "losses")
    _close(given["dz"], lin["dz"], "dz")
    dc = sum(d @ w for d, w in zip(given["dP"], wk))
    _close(torch.flip(dc, [1]), lin["dc"][:, k:], "dc from dP")
    assert float(lin["dc"][:, :k].abs().max()) == 0.0
    with pytest.raises(ValueError):
        O.criterion_forward_sparse(None, z, [torch.zeros(b, t_len, henc, dtype=torch.float64)] * k, ext, nn)
    assert np.asarray(ext).shape == (b * nn * (t_len - k),)
