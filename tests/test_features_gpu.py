"""Feature extraction on the MI355X (feature_loader.buildFeature, buildFeature_batch, buildFeature_device, seqNormalization, the
carried recurrent state) against what the reference's own feature_loader returned: tests/golden/g25_features.* (float64 runs of
the reference's classes, tools/make_golden_features.py).  Models: the checkpoint the reference wrote (hidden 32) and oracle/synth
parameters at hidden 256 / 512 (GRU, LSTM x2, GRU x2, transformer); the wide models' outputs are compared on the golden's 64
stored channels, shapes in full.

Tolerances: those test_reference_written_checkpoint_loads_into_hip_modules holds the same checkpoint to -- per case and span
max|got - ref| <= 2e-5 max|ref| (encoded), 5e-5 max|ref| (context)."""
import json
import os

import numpy as np
import pytest
import torch

import cpc2_amd
import features_probe as FP
from cpc2_amd.feature_loader import FeatureModule, buildFeature, buildFeature_batch, buildFeature_device, loadModel, seqNormalization

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "g25_features.json")) as _f:
    META = json.load(_f)
MODELS = ["h32"] + list(META["models"])
RECURRENT = ["h32"] + [m for m, cfg in META["models"].items() if cfg["ar"] != "transformer"]
TOL = {True: 2e-5, False: 5e-5}          # by get_encoded


@pytest.fixture(scope="module")
def arrays():
    a32 = np.load(os.path.join(GOLDEN, "g25_features.npz"), allow_pickle=False)
    aw = np.load(os.path.join(GOLDEN, "g25_features_wide.npz"), allow_pickle=False)
    return {"h32": a32, "wide": aw, "wave": torch.from_numpy(a32["wave"]).view(1, -1)}


_MODELS = {}


def _model(name):
    """The model of the golden's `name` on the GPU, built once."""
    if name in _MODELS:
        return _MODELS[name]
    if name == "h32":
        model, _, _ = loadModel([os.path.join(GOLDEN, "ref_checkpoint", "checkpoint_7.pt")])
    else:
        cfg = META["models"][name]
        h = cfg["hidden"]
        if cfg["ar"] == "transformer":
            from cpc2_amd.transformers import buildTransformerAR
            ar = buildTransformerAR(h, h, cfg["layers"], cfg["size_seq"], False)
        else:
            ar = cpc2_amd.CPCAR(h, h, False, cfg["layers"], mode=cfg["ar"])
        model = cpc2_amd.CPCModel(cpc2_amd.CPCEncoder(h), ar)
        sd = FP.wide_params(cfg)
        sd.update({k: v for k, v in model.state_dict().items() if k.endswith(".z") or k.endswith(".mask")})
        model.load_state_dict(sd)
    _MODELS[name] = model.to(DEV).eval()
    return _MODELS[name]


def _arr(arrays, name):
    return arrays["h32"] if name == "h32" else arrays["wide"]


def _channels(arrays, name):
    return None if name == "h32" else arrays["wide"][f"chan/{name}"]


def _run(arrays, c, seqNorm=None, reader=None):
    wave = arrays["wave"][:, c["start"]:c["start"] + c["n"]]
    maker = FeatureModule(_model(c["model"]), c["get_encoded"]).eval()
    seqNorm = c["seqNorm"] if seqNorm is None else seqNorm
    if reader is not None:
        return reader(maker, wave, strict=c["strict"], maxSizeSeq=c["maxSizeSeq"], seqNorm=seqNorm)
    if c["reader"] == "buildFeature":
        return buildFeature(maker, wave, strict=c["strict"], maxSizeSeq=c["maxSizeSeq"], seqNorm=seqNorm)
    return buildFeature_batch(maker, wave, strict=c["strict"], maxSizeSeq=c["maxSizeSeq"], seqNorm=seqNorm, batch_size=c["batch_size"])


def _stored(got, ch):
    g = got[0].double().numpy()
    return g if ch is None else g[:, ch]


def _cases(name, seqNorm):
    out = [c for c in META["cases"] if c["model"] == name and c["seqNorm"] == seqNorm]
    assert out
    return out


@pytest.mark.parametrize("name", MODELS)
def test_raw_features_match_the_references(arrays, name):
    """Every raw case of the model: the golden's shape exactly; per span max|got - ref| within the tolerance times the case's
    max|ref|.  The short-rest cases (a rest of 159 .. 399 samples fed on its own: 1 or 2 frames) are among them."""
    arr, ch = _arr(arrays, name), _channels(arrays, name)
    short = 0
    for c in _cases(name, False):
        got = _run(arrays, c)
        assert list(got.shape) == c["shape"], c["id"]
        assert got.device.type == "cpu"
        g, ref = _stored(got, ch), arr["val/" + c["id"]].astype(np.float64)
        tol, at, worst, last = TOL[c["get_encoded"]] * c["ref_max"], 0, 0.0, 0.0
        for per, kept in c["spans"]:
            last = float(np.abs(g[at:at + kept] - ref[at:at + kept]).max())
            worst = max(worst, last)
            at += kept
        assert at == ref.shape[0]
        print(f"G25 {c['id']}: |got - f64| {worst:.2e}, last span ({c['spans'][-1][0]} frames, {c['spans'][-1][1]} kept) {last:.2e}  "
              f"(the reference's f32 run: {c['f32_dist']:.2e}; bound {tol:.2e})")
        at = 0
        for i, (per, kept) in enumerate(c["spans"]):
            d = float(np.abs(g[at:at + kept] - ref[at:at + kept]).max())
            assert d <= tol, f"{c['id']} span {i}: {d:.3e} > {tol:.3e}"
            at += kept
        short += c["spans"][-1][0] <= 2
    assert short >= 2


@pytest.mark.parametrize("name", MODELS)
def test_seqnorm_features(arrays, name):
    """seqNorm divides by s = sqrt(var + 1e-8) over a span's frames; post-ReLU channels are often nearly constant within a chunk,
    so an error e of the raw features becomes 2 e (1 + |ref|) / s to first order: that is the bound, per element, with e the raw
    tolerance times max|raw ref| and s from the golden.  Independent of conditioning: the output must be seqNormalization, in
    f64, of the project's OWN raw span features within the same bound at e = 2^-22 max|raw| of the span and channel, and exactly
    0 where that maximum is 0."""
    arr, ch = _arr(arrays, name), _channels(arrays, name)
    for c in _cases(name, True):
        got = _run(arrays, c)
        assert list(got.shape) == c["shape"], c["id"]
        g, ref, std = _stored(got, ch), arr["val/" + c["id"]].astype(np.float64), arr["std/" + c["id"]]
        e = TOL[c["get_encoded"]] * c["raw_max"]
        own = _run(arrays, c, seqNorm=False)[0].double()
        gfull = got[0].double()
        at, worst, worst_own = 0, 0.0, 0.0
        assert len(std) == len(c["spans"])
        for i, (per, kept) in enumerate(c["spans"]):
            bound = 2 * e * (1 + np.abs(ref[at:at + kept])) / std[i]
            d = np.abs(g[at:at + kept] - ref[at:at + kept])
            worst = max(worst, float((d / bound).max()))
            assert np.all(d <= bound), f"{c['id']} span {i}: {float((d / bound).max()):.2f} of the bound"
            # the project's own raw span: the kept frames, or (strict tail) the whole last chunk run again
            if kept == per:
                span = own[at:at + per]
            else:
                tail = arrays["wave"][:, c["start"] + c["n"] - c["maxSizeSeq"]:c["start"] + c["n"]].view(1, 1, -1)
                with torch.no_grad():
                    span = FeatureModule(_model(name), c["get_encoded"]).eval()((tail, None))[0].double().cpu()
                assert span.shape[0] == per and torch.equal(span[per - kept:], own[at:at + kept]), f"{c['id']}: the tail is not reproducible"
            want = seqNormalization(span.unsqueeze(0))[0][per - kept:]
            s64 = torch.sqrt(span.var(dim=0) + 1e-8)
            e_own = 2.0 ** -22 * span.abs().max(dim=0)[0]
            bound_own = 2 * e_own * (1 + want.abs()) / s64
            d_own = (gfull[at:at + kept] - want).abs()
            assert bool((d_own <= bound_own).all()), f"{c['id']} span {i} (own raw features): {float((d_own / bound_own.clamp_min(1e-300)).max()):.2f} of the bound"
            assert bool((gfull[at:at + kept][:, e_own == 0] == 0).all())
            worst_own = max(worst_own, float((d_own / bound_own.clamp_min(1e-300)).max()))
            at += kept
        print(f"G25 {c['id']}: {worst:.3f} of the first-order bound, {worst_own:.3f} of the own-raw bound; |got - f64| "
              f"{float(np.abs(g - ref).max()):.2e}  (the reference's f32 run: {c['f32_dist']:.2e})")


@pytest.mark.parametrize("name", RECURRENT)
def test_keep_hidden_carries_the_state_across_chunks_and_files(arrays, name):
    """One keepHidden feature maker on file A, then B, then A again, chunk 10 000 (chunk borders inside frames): the recurrent
    state is never reset -- not between chunks, not between files -- so the third output differs from the first (by 0.12 .. 0.54
    in the golden) and all three must be the reference's."""
    rec = next(k for k in META["keepHidden"] if k["model"] == name)
    arr, ch = _arr(arrays, name), _channels(arrays, name)
    model = _model(name)
    assert rec["third_call_differs_from_first_by"] > 0.1
    model.gAR.keepHidden, model.gAR.hidden = True, None
    try:
        maker = FeatureModule(model, False).eval()
        outs = [buildFeature(maker, arrays["wave"][:, c["start"]:c["start"] + c["n"]], maxSizeSeq=rec["maxSizeSeq"]) for c in rec["calls"]]
    finally:
        model.gAR.keepHidden, model.gAR.hidden = False, None
    for c, got in zip(rec["calls"], outs):
        assert list(got.shape) == c["shape"], c["id"]
        d = float(np.abs(_stored(got, ch) - arr["val/" + c["id"]].astype(np.float64)).max())
        print(f"G25 {c['id']}: |got - f64| {d:.2e}  (the reference's f32 run: {c['f32_dist']:.2e}; bound {5e-5 * c['ref_max']:.2e})")
        assert d <= 5e-5 * c["ref_max"], f"{c['id']}: {d:.3e}"
    assert float((outs[2] - outs[0]).abs().max()) > 0.1


@pytest.mark.parametrize("cid", ["h32/bf/ctx/strict/norm/full", "gru256/bf/ctx/loose/norm/full", "gru512x2/bf/enc/loose/raw/rest319"])
def test_build_feature_device_equals_build_feature_bit_for_bit(arrays, cid):
    c = next(c for c in META["cases"] if c["id"] == cid)
    host = _run(arrays, c)
    dev = _run(arrays, c, reader=buildFeature_device)
    assert dev.device.type == "cuda" and host.device.type == "cpu"
    assert torch.equal(dev.cpu(), host)


@pytest.mark.parametrize("name", ["h32", "gru256", "gru512x2"])
def test_lengths_that_leave_no_frame_are_refused(arrays, name):
    """158 samples leave no frame: a Python exception from the shape query, before any launch, where the reference raises too --
    alone, and as the non-strict rest of a file."""
    maker = FeatureModule(_model(name), True).eval()
    with pytest.raises(ValueError, match="encoder shape query"):
        maker((arrays["wave"][:, :158].view(1, 1, -1), None))
    with pytest.raises(ValueError, match="encoder shape query"):
        buildFeature(maker, arrays["wave"][:, :4000 + 158], maxSizeSeq=4000)
    assert buildFeature(maker, arrays["wave"][:, :4000 + 159], maxSizeSeq=4000).shape[1] == 25 + 1
    torch.cuda.synchronize()
