"""feature_loader's readers against what the reference's did (tests/golden/g25_features.*, tools/make_golden_features.py), on the
CPU: the plan -- chunks, rest, strict tail, batching, the short-rest rule -- in integers through a probe feature maker, and
seqNormalization on the reference's recorded raw spans."""
import json
import os

import numpy as np
import pytest
import torch

import features_probe as FP
from cpc2_amd.feature_loader import buildFeature, buildFeature_batch, seqNormalization

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def g25():
    with open(os.path.join(GOLDEN, "g25_features.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, "g25_features.npz"), allow_pickle=False), \
        np.load(os.path.join(GOLDEN, "g25_features_wide.npz"), allow_pickle=False)


def _read(reader, maker, wave, strict, C, seqNorm, bs):
    if reader == "buildFeature":
        return buildFeature(maker, wave, strict=strict, maxSizeSeq=C, seqNorm=seqNorm)
    return buildFeature_batch(maker, wave, strict=strict, maxSizeSeq=C, seqNorm=seqNorm, batch_size=bs)


def test_probe_frame_rule_is_the_librarys():
    from cpc2_amd import _lib
    lib = _lib.load()
    for length in (159, 160, 319, 320, 399, 400, 4000, 8000, 10000, 20480, 64000):
        assert FP.frames(length) == lib.cpc_encoder_frames(length)
    assert FP.frames(158) == 0 and FP.frames(159) == 1
    # the shortest input: 159 samples for every kernel form; one sample less is refused by the size queries (no launch follows)
    for length in range(1, 170):
        assert lib.cpc_encoder_frames(length) == max(FP.frames(length), 0) == (1 if length >= 159 else 0)
    for hidden in (32, 64, 128, 256, 512):
        for n in (1, 3):
            assert lib.cpc_encoder_saved_bytes(n, 159, hidden) > 0 and lib.cpc_encoder_scratch_bytes(n, 159, hidden) > 0
            assert lib.cpc_encoder_saved_bytes(n, 158, hidden) == 0 and lib.cpc_encoder_scratch_bytes(n, 158, hidden) == 0
            assert lib.cpc_encoder_saved_bytes(n, 1, hidden) == 0


def test_readers_follow_the_references_plan_exactly(g25):
    """Every case of the provenance sweep: the same frames, from calls of the same length and row count; where the reference
    raised (a rest that leaves no frame fed on its own, a file the batched reader finds nothing in), so does this."""
    meta, arr, _ = g25
    cases = FP.sweep_cases()
    assert len(cases) == meta["provenance"]["cases"] == 384
    raised = meta["provenance"]["raised"]
    probe = FP.ProbeMaker()
    seen_raise = 0
    for case in cases:
        reader, C, strict, bs, n = case
        key = FP.sweep_key(case)
        wave = torch.arange(n, dtype=torch.float32).view(1, -1)
        if key in raised:
            assert key not in arr.files
            with pytest.raises((ValueError, RuntimeError)):
                _read(reader, probe, wave, strict, C, False, bs)
            seen_raise += 1
            continue
        got = FP.encode(_read(reader, probe, wave, strict, C, False, bs))
        assert got.shape == arr[key].shape and np.array_equal(got, arr[key]), f"{key}:\n{got}\nreference:\n{arr[key]}"
    assert seen_raise == len(raised) == 24


def test_seqnorm_is_applied_per_call_before_the_tail_cut(g25):
    """The sweep's seqNorm cases: the probe's sample channel normalised over each call's frames (the whole chunk of a strict
    tail, of which only the last frames are kept); the two constant channels become 0.  Values are O(1): 1e-5 is ~50 ulp."""
    meta, arr, _ = g25
    probe = FP.ProbeMaker()
    assert len(meta["provenance"]["seqnorm"]) == 8
    for c in meta["provenance"]["seqnorm"]:
        wave = torch.arange(c["n"], dtype=torch.float32).view(1, -1)
        got = _read(c["reader"], probe, wave, c["strict"], c["maxSizeSeq"], True, c["batch_size"])[0].numpy()
        ref = arr[c["key"]]
        assert got.shape == ref.shape, c["key"]
        assert np.abs(ref).max() > 1.0 and np.all(ref[:, 1:] == 0)
        assert np.abs(got.astype(np.float64) - ref).max() <= 1e-5, c["key"]


def test_seq_normalization_on_the_references_raw_spans(g25):
    """seqNormalization of the golden's raw spans (f64 run, rounded to f32) against the golden's normalised spans.  The division
    by s = sqrt(var + 1e-8) amplifies an input error e to 2 e (1 + |ref|) / s (first order); e = 2^-22 max|raw| of the span and
    channel covers the rounding of the stored input (2^-24) and the f32 arithmetic; a constant-zero channel must give exactly 0."""
    meta, a32, aw = g25
    by_id = {c["id"]: c for c in meta["cases"]}
    done = 0
    for c in meta["cases"]:
        if not c["seqNorm"] or "raw_of" not in c:
            continue
        arr = a32 if c["model"] == "h32" else aw
        raw, ref, std = arr["val/" + c["raw_of"]], arr["val/" + c["id"]], arr["std/" + c["id"]]
        assert by_id[c["raw_of"]]["spans"] == c["spans"] and not by_id[c["raw_of"]]["seqNorm"]
        at = 0
        for i, (per, kept) in enumerate(c["spans"]):
            span = arr["rawtail/" + c["id"]] if kept < per else raw[at:at + per]
            assert span.shape[0] == per
            got = seqNormalization(torch.from_numpy(span).unsqueeze(0))[0][per - kept:].double().numpy()
            want = ref[at:at + kept].astype(np.float64)
            e = 2.0 ** -22 * np.abs(span).max(axis=0)
            bound = 2 * e * (1 + np.abs(want)) / std[i]
            assert np.all(np.abs(got - want) <= bound), f"{c['id']} span {i}: {np.abs(got - want).max():.2e}"
            assert np.all(got[:, e == 0] == 0)
            at += kept
            done += 1
        assert at == ref.shape[0]
    assert done >= 8 * 4
