"""Audio augmentation without a GPU: the fp64 statements of tests/augment_oracle.py against the reference's recorded outputs
(tests/golden/g24_augment.npz, tools/make_golden_augment.py), augmentation_factory against the reference's recorded dispatch
(g24_augment_factory.json), what the command line lets through and refuses, and the host side of a pack -- its plan."""
import json
import os
import random
import types

import numpy as np
import pytest
import torch

import augment_oracle as AO
from cpc2_amd import data_augmentation as da
from cpc2_amd import dataset as ds
from cpc2_amd import train as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DB = os.path.join(ROOT, "tests", "golden", "test_db")
MISSING = os.path.join(ROOT, "tests", "golden", "no_such_data_set")
TOL = 2e-6          # the project's kernel-parity bound, absolute on peak-normalised outputs
W = 2048


# ----------------------------------------------------------------------------- 1. the oracle against the reference's recordings
def test_oracle_reproduces_the_recorded_additive_outputs(golden):
    g = golden("g24_augment.npz")
    count = int(g["add_count"])
    assert count >= 5
    zero_noise = zero_speech = False
    for i in range(count):
        x, noise, ref = g[f"add{i}_x"], g[f"add{i}_noise"], g[f"add{i}_out"]
        lo, hi = g[f"add{i}_snr"]
        np.random.seed(int(g[f"add{i}_seed"]))
        snr = (hi - lo) * np.random.random_sample() + lo
        got = AO.additive(x, noise, AO.gain_of(snr))
        err = float(np.abs(got - ref).max())
        print(f"additive case {i}: |oracle - reference| = {err:.2e}")
        assert np.isfinite(got).all() and np.isfinite(ref).all()
        assert err <= TOL, (i, err)
        zero_noise |= not noise.any()
        zero_speech |= not x.any()
    assert zero_noise and zero_speech


def test_oracle_and_package_normalisations_match_the_recordings(golden):
    g = golden("g24_augment.npz")
    assert np.abs(AO.peak_norm(g["pn_in"]) - g["pn_out"]).max() <= TOL
    assert np.abs(AO.peak_norm(g["pk_in"]) - g["pk_out"]).max() <= TOL
    assert np.abs(AO.energy_norm(g["en_in"]) - g["en_out"]).max() <= TOL
    assert not g["en_zero_out"].any() and not AO.energy_norm(np.zeros((1, 512))).any()
    # the package's host statements are the reference's expressions
    assert np.array_equal(ds.PeakNorm()(torch.from_numpy(g["pn_in"])).numpy(), g["pn_out"])
    assert np.array_equal(da.peak_normalization(torch.from_numpy(g["pk_in"])).numpy(), g["pk_out"])
    assert np.array_equal(da.energy_normalization(torch.from_numpy(g["en_in"])).numpy(), g["en_out"])


# ----------------------------------------------------------------------------- fixtures
@pytest.fixture()
def noise_db(tmp_path):
    return AO.make_noise_db(tmp_path / "noise")


@pytest.fixture()
def ir_db(tmp_path):
    return AO.make_ir_db(tmp_path / "irs")


def _noise_dataset(noise_db, window=W, augmentation=None, meta=False):
    seqs, _ = ds.findAllSeqs(noise_db, extension=".wav", speaker_level=0)
    return ds.AudioBatchData(noise_db, window, seqs, None, 1, transform=ds.PeakNorm(), augment_past=meta, augmentation=augmentation,
                             keep_temporality=False, past_equal_future=meta, device="cpu")


def _speech_dataset(window=W, **kw):
    seqs, speakers = ds.findAllSeqs(DB, extension=".flac")
    seqs = sorted(seqs, key=lambda s: s[1])
    return ds.AudioBatchData(DB, window, seqs, None, len(speakers), device="cpu", **kw)


# ----------------------------------------------------------------------------- 2. the factory's dispatch
BUILT = {"AdditiveNoiseAugment", "NaturalReverb", "TimeDropoutAugment", "CombinedTransforms"}


def test_augmentation_factory_matches_the_recorded_dispatch(noise_db, ir_db, capsys):
    with open(os.path.join(ROOT, "tests", "golden", "g24_augment_factory.json")) as fh:
        table = json.load(fh)
    assert len(table) >= 20
    noise = _noise_dataset(noise_db)
    seen = set()
    for tag, case in table.items():
        values = dict(case["args"])
        assert values["pathImpulseResponses"] == "$IR"
        values["pathImpulseResponses"] = ir_db
        args = types.SimpleNamespace(**values)
        want = case["result"]

        def build():
            return da.augmentation_factory(args, noise if case["noise_dataset"] else None, applied_on_noise=case["applied_on_noise"])

        if tag == "type_none":
            # documented deviation: the reference's factory raises on the one-element list ['none'] (it compares the list with
            # the string); here `--augment_type none` is the same as no type
            assert want == {"error": "RuntimeError", "message": "Unknown augment_type = none"}
            assert build() is None
            continue
        if "error" in want:
            with pytest.raises(RuntimeError) as err:
                build()
            assert type(err.value).__name__ == want["error"] and str(err.value) == want["message"], tag
            seen.add("error")
            continue
        names = [want["class"]] + [p for p in want.get("parts", []) if p is not None]
        if want["class"] is not None and not set(names) <= BUILT:
            # a type the reference builds on sox: refused by name, with the refusal's fixed opening
            with pytest.raises(NotImplementedError, match="--augment_past / --augment_future with --augment_type"):
                build()
            seen.add("unbuilt")
            continue
        got = build()
        if want["class"] is None:
            assert got is None, tag
            seen.add("none")
            continue
        assert type(got).__name__ == want["class"], tag
        seen.add(want["class"])
        if "parts" in want:
            assert [None if t is None else type(t).__name__ for t in got.transfors_cfgs] == want["parts"], tag
        if "batch_wise" in want:
            assert got.batch_wise == want["batch_wise"], tag
        if "sampling" in want:
            assert got.sampling == want["sampling"] and got.batchSize == want["batchSize"], tag
    assert seen >= BUILT | {"error", "unbuilt", "none"}
    assert "Found 3 files for natural reverberation" in capsys.readouterr().out


# ----------------------------------------------------------------------------- 3. the command line
def _args(*flags):
    return tr.parseArgs(["--pathDB", MISSING, "--nGPU", "0", "--random_seed", "0"] + list(flags))


@pytest.mark.parametrize("flags", [
    ["--augment_past", "--augment_type", "additive", "--pathDBNoise", "noise"],
    ["--augment_past", "--augment_type", "natural_reverb", "--pathImpulseResponses", "irs"],
    ["--augment_future", "--augment_type", "time_dropout"],
    ["--augment_past", "--augment_future", "--augment_type", "additive", "natural_reverb", "--pathDBNoise", "noise",
     "--pathImpulseResponses", "irs"],
    ["--augment_past", "--past_equal_future", "--augment_type", "natural_reverb", "additive", "time_dropout", "--pathDBNoise", "noise",
     "--pathImpulseResponses", "irs", "--meta_aug", "--meta_aug_type", "natural_reverb"],
    ["--augment_past", "--augment_type", "none"],
    ["--augment_type", "pitch"],                                   # no half is augmented: nothing is asked for
], ids=lambda f: " ".join(f))
def test_refuse_unsupported_lets_the_built_types_through(flags):
    tr.refuseUnsupported(_args(*flags))


SOX = ["pitch", "pitch_quick", "pitch_deropout", "artificial_reverb", "artificial_reverb_dropout", "bandreject"]


@pytest.mark.parametrize("types_", [[t] for t in SOX] + [["additive", "pitch"], ["bandreject", "natural_reverb", "time_dropout"]],
                         ids=lambda t: "+".join(t))
def test_every_sox_type_is_refused_by_name_before_the_data_set_is_opened(types_, monkeypatch):
    opened = []
    monkeypatch.setattr(ds, "findAllSeqs", lambda *a, **k: opened.append(a) or ([], []))
    flags = ["--augment_past", "--augment_type"] + types_ + ["--pathDBNoise", MISSING, "--pathImpulseResponses", MISSING]
    with pytest.raises(NotImplementedError, match=r"--augment_past / --augment_future with --augment_type") as err:
        tr.main(["--pathDB", MISSING, "--nGPU", "0", "--random_seed", "0"] + flags)
    for t in types_:
        if t in SOX:
            assert t in str(err.value).split(":", 1)[1]
    assert "additive, natural_reverb, time_dropout" in str(err.value)          # names what is built
    assert not opened and not os.path.exists(MISSING)


def test_additive_without_a_noise_data_set_raises_before_the_speech_is_loaded(monkeypatch, tmp_path, capsys):
    built = []
    monkeypatch.setattr(ds, "AudioBatchData", lambda *a, **k: built.append(a) or (_ for _ in ()).throw(AssertionError("data loaded")))
    for types_ in (["additive"], ["natural_reverb", "additive"]):
        with pytest.raises(RuntimeError, match="^Noise dataset is needed for the additive noise$"):
            tr.main(["--pathDB", DB, "--nGPU", "0", "--random_seed", "0", "--path_cache", str(tmp_path / "cache.txt"),
                     "--augment_past", "--augment_type"] + types_ + ["--pathImpulseResponses", MISSING])
    assert not built
    with pytest.raises(RuntimeError, match="^Noise dataset is needed for the additive noise$"):
        da.get_augment("additive", noise_dataset=None)


def test_argument_errors_hold():
    with pytest.raises(ValueError, match="when past sequence is augmented"):
        _speech_dataset(past_equal_future=True)
    with pytest.raises(ValueError, match="when past sequence is augmented"):
        _speech_dataset(past_equal_future=True, augment_future=True, augmentation=da.TimeDropoutAugment(10))
    with pytest.raises(ValueError, match="--meta_aug_type without having activated --meta_aug"):
        _args("--meta_aug_type", "natural_reverb")
    with pytest.raises(ValueError, match="--meta_aug, but you haven't specified meta_aug_type"):
        _args("--meta_aug")
    with pytest.raises(NotImplementedError, match="PeakNorm"):
        _speech_dataset(transform=lambda x: x)
    with pytest.raises(ValueError, match="--t_ms 0"):
        da.TimeDropoutAugment(0)
    assert da.TimeDropoutAugment(1).max_frames == 16 and da.TimeDropoutAugment(100).max_frames == 1600


def test_impulse_response_at_another_rate_is_refused_by_name(tmp_path, capsys):
    root = AO.make_ir_db(tmp_path / "irs")
    AO.write_wav(tmp_path / "irs" / "hall_32k.wav", np.exp(-np.arange(100) / 10.0), rate=32000)
    with pytest.raises(ValueError, match=r"hall_32k\.wav.*32000 Hz.*--ir_sample_rate 16000"):
        da.NaturalReverb(root, 1.0, 4, sr=16000, device="cpu")
    assert "Found 4 files for natural reverberation" in capsys.readouterr().out
    with pytest.raises(ValueError, match=r"room_\d\.wav.*16000 Hz.*--ir_sample_rate 32000"):
        da.NaturalReverb(root, 1.0, 4)                             # the class's own default rate, as in the reference
    ok = da.NaturalReverb(AO.make_ir_db(tmp_path / "irs16"), 1.0, 4, sr=16000, device="cpu")
    assert sorted(ok.ir_len.tolist()) == [257, 1200, 4000]
    assert ok.ir_data.numel() == 257 + 1200 + 4000 and ok.ir_off.tolist() == [0] + np.cumsum(ok.ir_len)[:-1].tolist()


# ----------------------------------------------------------------------------- 4. a pack's plan
def _seed(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def _pack(seed, noise_db, ir_db, temporal=False, batch_wise=False, batch=4, meta=False, future=False):
    """Everything rebuilt from the seeds: noise data set, transforms, speech data set, the loader's plan of the first pack."""
    _seed(seed)
    meta_aug = da.NaturalReverb(ir_db, 0.7, batch, sr=16000, batch_wise=False, device="cpu") if meta else None
    noise = _noise_dataset(noise_db, augmentation=meta_aug, meta=meta)
    kw = dict(noise_dataset=noise, additive_noise_snr_min=5.0, additive_noise_snr_max=20.0, batchSize=batch,
              additive_noise_sampling="temporalsamespeaker" if temporal else "uniform", impulse_response_prob=0.6,
              pathImpulseResponses=ir_db, ir_sample_rate=16000, ir_batch_wise=batch_wise, t_ms=40)
    aug = da.CombinedTransforms(["additive", "natural_reverb", "time_dropout"], **kw)
    speech = _speech_dataset(augment_past=True, augment_future=future, augmentation=aug)
    loader = speech.getDataLoader(batch, "uniform", True)
    batches, plans = loader.pack_plan()
    return types.SimpleNamespace(noise=noise, aug=aug, speech=speech, batches=batches, plans=plans)


def _same(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a if k not in ("_dev", "noise_data"))
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and np.array_equal(a, b)
    return a == b


@pytest.mark.parametrize("temporal", [False, True], ids=["uniform", "temporalsamespeaker"])
def test_a_packs_plan_is_a_pure_function_of_the_seeds(noise_db, ir_db, temporal, capsys):
    one = _pack(5, noise_db, ir_db, temporal=temporal, meta=True, future=True)
    two = _pack(5, noise_db, ir_db, temporal=temporal, meta=True, future=True)
    other = _pack(6, noise_db, ir_db, temporal=temporal, meta=True, future=True)
    assert one.batches == two.batches and _same(one.plans, two.plans)
    assert not _same(one.plans, other.plans)
    n = sum(len(b) for b in one.batches)
    assert n > 100
    for plan in one.plans:                                         # past and future: draws of their own
        add, rev, drop = plan["parts"]
        assert plan["n"] == add["n"] == rev["n"] == drop["n"] == n
        # noise offsets: inside the noise pack, and under temporal sampling (remove_artefacts) inside one noise file
        total = one.noise.data.numel()
        off = add["noise_off"]
        assert off.min() >= 0 and (off + W).max() <= total
        if temporal:
            bounds = np.asarray(one.noise.seqLabel)
            file_of = np.searchsorted(bounds, off, side="right") - 1
            assert (off + W <= bounds[file_of + 1]).all()
        assert (add["snr"] >= 5.0).all() and (add["snr"] <= 20.0).all() and len(set(add["snr"].tolist())) == n
        assert np.allclose(add["gain"], 10.0 ** (-add["snr"] / 20.0), rtol=1e-6)
        assert add["noise_peak_norm"] is True and add["meta"]["kind"] == "natural_reverb" and add["meta"]["n"] == n
        # dropout spans stay inside the window
        assert (drop["length"] >= 0).all() and (drop["length"] < 640).all() and (drop["start"] >= 0).all()
        assert (drop["start"] + drop["length"] <= W).all() and drop["length"].max() > 320
        # the probability test skips some convolutions (length 0) and keeps others
        skipped = rev["ir_len"] == 0
        assert 0.2 < skipped.mean() < 0.6 and ((rev["ir_index"] == -1) == skipped).all()
        assert set(rev["ir_len"][~skipped].tolist()) == {257, 1200, 4000}
    assert not _same(one.plans[0], one.plans[1])
    # window order, past before future: the two halves take alternate noise windows, SNRs and dropout spans from one stream
    past, future = one.plans[0]["parts"][0], one.plans[1]["parts"][0]
    assert not set(past["snr"].tolist()) & set(future["snr"].tolist())
    if temporal:                                                   # consecutive noise windows of one file: past, future, past, ...
        step = future["noise_off"] - past["noise_off"]
        assert (step == W).mean() > 0.8


def test_batch_wise_impulse_responses_change_every_batch_size_windows(ir_db, capsys):
    _seed(3)
    rev = da.NaturalReverb(ir_db, 1.0, 4, sr=16000, batch_wise=True, device="cpu")
    plan = rev.plan(64, W, "cpu")
    blocks = plan["ir_index"].reshape(16, 4)
    assert (blocks == blocks[:, :1]).all() and (blocks >= 0).all()          # one response per batchSize consecutive windows
    assert len(set(blocks[:, 0].tolist())) == 3                             # ... drawn again for every block
    assert (np.diff(blocks[:, 0]) != 0).sum() >= 5
    _seed(3)
    again = da.NaturalReverb(ir_db, 1.0, 4, sr=16000, batch_wise=True, device="cpu").plan(64, W, "cpu")
    assert np.array_equal(plan["ir_index"], again["ir_index"])
    _seed(3)
    seq = da.NaturalReverb(ir_db, 1.0, 4, sr=16000, batch_wise=False, device="cpu").plan(64, W, "cpu")
    assert (np.diff(seq["ir_index"].reshape(16, 4), axis=1) != 0).any()      # sequence-wise: a draw per window


def test_first_numpy_draw_of_a_single_call_is_the_snr(noise_db, golden):
    """After np.random.seed(s) the reference's AdditiveNoiseAugment.__call__ draws the SNR first (g24 relies on it)."""
    noise = _noise_dataset(noise_db)
    _seed(11)
    aug = da.AdditiveNoiseAugment(noise, 5.0, 20.0, 4, "uniform")
    np.random.seed(3)
    plan = aug.plan(1, W, "cpu")
    np.random.seed(3)
    assert plan["snr"][0] == 15.0 * np.random.random_sample() + 5.0


def test_augmented_loader_has_no_cpu_fallback(noise_db, ir_db, capsys):
    pack = _pack(1, noise_db, ir_db)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        next(iter(pack.speech.getDataLoader(4, "uniform", True)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        da.TimeDropoutAugment(10)(torch.zeros(1, W))
