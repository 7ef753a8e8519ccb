"""The `pitch_wsola` augmentation without a GPU: the float64 statement of tests/pitch_oracle.py does what a pitch shift does (a
sine comes out at 440 r Hz with its energy), its edge cases, the draws of PitchShiftAugment (the reference's one
np.random.randint(-shift_max, shift_max) per window), the host tables of a sealed plan, and the way from the command line to the
transform."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

import augment_oracle as AO
import pitch_oracle as PO
from cpc2_amd import data_augmentation as da
from cpc2_amd import dataset as ds
from cpc2_amd import feature_loader as fl
from cpc2_amd import train as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISSING = os.path.join(ROOT, "tests", "golden", "no_such_data_set")
FS = 16000


# ----------------------------------------------------------------------------- the statement shifts the pitch
def _sine(w, hz=440.0, amp=0.5):
    return (amp * np.sin(2 * np.pi * hz * np.arange(w) / FS)).astype(np.float32)


@pytest.mark.parametrize("cents", [300, -300, 57, -1])
def test_a_sine_comes_out_at_the_shifted_frequency_with_its_energy(cents):
    w = 20480
    y, q, bound = PO.pitch(_sine(w), cents)
    spectrum = np.abs(np.fft.rfft(y * np.hanning(w), 8 * w))
    peak = np.argmax(spectrum) * FS / (8 * w)
    rms = float(np.sqrt(np.mean(y ** 2)))
    print(f"cents={cents}: peak {peak:.2f} Hz (440 r = {440 * PO.ratio_of(cents):.2f}), rms {rms:.4f}, {len(q)} segments")
    assert abs(peak - 440.0 * PO.ratio_of(cents)) <= 1.0
    assert abs(rms - 0.3536) <= 0.02 * 0.3536
    assert 16 <= len(q) <= 22 and len(q) == PO.segments(w, cents)
    assert np.isfinite(bound).all() and bound.max() < 1e-5


def test_zero_cents_returns_the_window():
    x = (0.1 * np.random.RandomState(0).standard_normal(2048)).astype(np.float32)
    y, q, bound = PO.pitch(x, 0)
    assert np.array_equal(y, x.astype(np.float64)) and not bound.any()
    assert np.array_equal(q, np.arange(len(q)) * PO.HO)          # r = 1 and the tail of a segment is what follows it: cost 0 at d = R // 2


SEGMENTS = {-300: {1: 1, 191: 1, 1311: 1, 1312: 1, 1313: 2, 2431: 2, 2432: 2, 2433: 2},
            300: {1: 1, 191: 1, 1311: 2, 1312: 2, 1313: 2, 2431: 3, 2432: 3, 2433: 3}}


@pytest.mark.parametrize("cents", [-300, 300])
@pytest.mark.parametrize("w", [1, 191, 1311, 1312, 1313, 2431, 2432, 2433])
def test_short_and_odd_windows_give_finite_output_and_the_expected_segment_counts(w, cents):
    x = (0.1 * np.random.RandomState(w).standard_normal(w)).astype(np.float32)
    y, q, bound = PO.pitch(x, cents)
    assert y.shape == (w,) and np.isfinite(y).all() and np.isfinite(bound).all()
    assert len(q) == SEGMENTS[cents][w] == PO.segments(w, cents) == da.pitch_segments(w, PO.ratio_of(cents))
    # the count covers the last tap of the last output and is no more than one segment beyond it
    r = PO.ratio_of(cents)
    last_tap = int(np.floor((w - 1) * r + PO.L / PO.cutoff_of(r)))
    assert last_tap < len(q) * PO.HO and (len(q) - 1) * PO.HO <= last_tap + PO.TAP_GUARD + 2


def test_an_all_zero_window_gives_zeros_and_the_first_candidate_everywhere():
    for cents in (-300, 123):
        y, q, bound = PO.pitch(np.zeros(4096, np.float32), cents)
        assert not y.any() and not bound.any() and len(q) >= 3
        assert np.array_equal(q[1:], PO.nominal_starts(cents, len(q))[1:] - PO.R // 2) and q[0] == 0


def test_a_tie_goes_to_the_lowest_candidate_and_a_match_is_found():
    # a constant window: every candidate inside it costs 0, the first of them wins
    q = PO.search(np.full(8192, 0.25, np.float32), 100)
    assert np.array_equal(q[1:3], PO.nominal_starts(100, len(q))[1:3] - PO.R // 2)
    # a window that repeats with a period below R: the template recurs among the candidates, and the start found is whole periods
    # away from where the previous segment goes on (away from the window's end, where zeros are read)
    x = np.tile(np.random.RandomState(3).standard_normal(100).astype(np.float32), 90)
    q = PO.search(x, -200)
    assert len(q) == 8 and all((q[j] - (q[j - 1] + PO.HO)) % 100 == 0 for j in range(1, len(q) - 1))


# ----------------------------------------------------------------------------- the draws
def test_draw_one_is_one_randint_per_window():
    aug = da.PitchShiftAugment(300)
    np.random.seed(11)
    got = [aug.draw_one(20480) for _ in range(50)]
    after = np.random.random_sample()
    np.random.seed(11)
    want = [int(np.random.randint(-300, 300)) for _ in range(50)]
    assert got == want and all(isinstance(c, int) for c in got) and after == np.random.random_sample()
    assert min(got) < -100 and max(got) > 100
    aug = da.PitchShiftAugment(7.0)                              # (the command line's --shift_max is a float)
    np.random.seed(12)
    got = [aug.draw_one(64) for _ in range(200)]
    np.random.seed(12)
    assert got == [int(np.random.randint(-7, 7)) for _ in range(200)] and set(got) == set(range(-7, 7))


@pytest.mark.parametrize("order", [["pitch_wsola", "time_dropout"], ["time_dropout", "none", "pitch_wsola"]], ids="+".join)
def test_combined_transforms_draw_in_the_order_of_the_parts(order):
    w = 20480
    aug = da.CombinedTransforms(order, shift_max=250, t_ms=100)
    assert [type(t).__name__ for t in aug._parts] == [{"pitch_wsola": "PitchShiftAugment", "time_dropout": "TimeDropoutAugment"}[t]
                                                      for t in order if t != "none"]
    np.random.seed(13)
    got = [aug.draw_one(w) for _ in range(20)]
    np.random.seed(13)
    for entry in got:
        want = []
        for t in order:
            if t == "pitch_wsola":
                want.append(int(np.random.randint(-250, 250)))
            elif t == "time_dropout":
                length = int(np.random.randint(0, 1600))
                want.append((int(np.random.randint(0, max(1, w - length))), length))
        assert entry == tuple(want)
    plan = aug.seal(got, torch.device("cpu"))
    kinds = [p["kind"] for p in plan["parts"]]
    assert kinds == [t for t in order if t != "none"]
    pitch_part = plan["parts"][kinds.index("pitch_wsola")]
    assert pitch_part["cents"].tolist() == [e[kinds.index("pitch_wsola")] for e in got]


# ----------------------------------------------------------------------------- the plan's tables
@pytest.mark.parametrize("w", [1, 2048, 20480])
def test_seal_builds_the_statements_tables(w):
    aug = da.PitchShiftAugment(1200)
    cents = [-1200, -300, -1, 0, 1, 57, 300, 1200, 1199]
    plan = aug.seal(cents, torch.device("cpu"), window=w)
    want = PO.tables(cents, w)
    assert plan["kind"] == "pitch_wsola" and plan["n"] == len(cents) and plan["window"] == w and plan["cents_bound"] == 1200
    for key, dtype in (("cents", np.int32), ("ratio", np.float64), ("cutoff", np.float64), ("nominal", np.int32)):
        assert plan[key].dtype == dtype and np.array_equal(plan[key], want[key]), key
        assert torch.equal(plan["_dev"][key], torch.from_numpy(want[key])), key
    assert plan["nominal"].shape == (len(cents), PO.segments(w, 1200))
    assert plan["ratio"][0] == 0.5 and plan["ratio"][3] == 1.0 and plan["ratio"][7] == 2.0
    assert plan["cutoff"][0] == 0.99 and plan["cutoff"][7] == 0.99 / 2.0
    # without window=: the window of the last draw
    np.random.seed(1)
    entries = [aug.draw_one(w) for _ in range(3)]
    again = aug.seal(entries, torch.device("cpu"))
    assert again["window"] == w and np.array_equal(again["nominal"], PO.tables(entries, w)["nominal"])
    with pytest.raises(ValueError, match="window length"):
        da.PitchShiftAugment(10).seal([1], torch.device("cpu"))


@pytest.mark.parametrize("bad,match", [(0, "at least 1 cent"), (-5, "at least 1 cent"), (0.5, "whole number"), (300.5, "whole number"),
                                       (1201, "at most 1200"), (5000.0, "at most 1200")])
def test_every_shift_max_refusal_names_the_flag(bad, match):
    with pytest.raises(ValueError, match=match) as err:
        da.PitchShiftAugment(bad)
    assert str(err.value).startswith(f"--shift_max {bad}")
    with pytest.raises(ValueError, match=match):
        da.get_augment("pitch_wsola", shift_max=bad)
    assert da.PitchShiftAugment(1).shift_max == 1 and da.PitchShiftAugment(1200.0).shift_max == 1200
    with pytest.raises(ValueError, match="at most 1200"):
        da.pitch_tables([1201], 64)


# ----------------------------------------------------------------------------- from the command line to the transform
def _args(*flags):
    args = tr.parseArgs(["--pathDB", MISSING, "--nGPU", "0", "--random_seed", "0"] + list(flags))
    args.nGPU = 1                                       # (parseArgs checks --nGPU against the devices present; the factory multiplies by it)
    return args


@pytest.mark.parametrize("flags", [
    ["--augment_past", "--augment_type", "pitch_wsola"],
    ["--augment_past", "--augment_type", "pitch_wsola", "time_dropout"],
    ["--augment_past", "--augment_type", "additive", "pitch_wsola", "--pathDBNoise", "noise"],
], ids=" ".join)
def test_refuse_unsupported_lets_pitch_wsola_through(flags):
    tr.refuseUnsupported(_args(*flags))


def test_the_lists_of_types():
    from cpc2_amd.cpc_default_config import AUGMENT_TYPES
    assert da.BUILT_TYPES == ("additive", "natural_reverb", "time_dropout", "pitch_wsola")
    assert "pitch_wsola" in AUGMENT_TYPES and "pitch_wsola" not in da.UNBUILT_TYPES
    assert {"pitch", "pitch_quick", "pitch_dropout", "pitch_deropout", "bandreject", "artificial_reverb",
            "artificial_reverb_dropout"} <= set(da.UNBUILT_TYPES)
    assert "additive, natural_reverb, time_dropout, pitch_wsola" in da.unbuilt_message(["pitch"])


def test_the_factory_builds_the_transform_and_its_combinations(tmp_path, capsys):
    got = da.augmentation_factory(_args("--augment_past", "--augment_type", "pitch_wsola"))
    assert type(got) is da.PitchShiftAugment and got.shift_max == 300 and not got.inplace
    got = da.augmentation_factory(_args("--augment_future", "--augment_type", "pitch_wsola", "--shift_max", "120"))
    assert type(got) is da.PitchShiftAugment and got.shift_max == 120
    got = da.augmentation_factory(_args("--augment_past", "--augment_type", "pitch_wsola", "time_dropout", "--shift_max", "50",
                                        "--t_ms", "20"))
    assert type(got) is da.CombinedTransforms
    assert [type(t) for t in got.transfors_cfgs] == [da.PitchShiftAugment, da.TimeDropoutAugment]
    assert got.transfors_cfgs[0].shift_max == 50 and got.transfors_cfgs[1].max_frames == 320
    noise_db = AO.make_noise_db(tmp_path / "noise")
    seqs, _ = ds.findAllSeqs(noise_db, extension=".wav", speaker_level=0)
    noise = ds.AudioBatchData(noise_db, 2048, seqs, None, 1, transform=ds.PeakNorm(), keep_temporality=False, device="cpu")
    got = da.augmentation_factory(_args("--augment_past", "--augment_type", "additive", "pitch_wsola", "--pathDBNoise", noise_db),
                                  noise)
    assert [type(t) for t in got.transfors_cfgs] == [da.AdditiveNoiseAugment, da.PitchShiftAugment]
    assert da.augmentation_factory(_args("--augment_type", "pitch_wsola")) is None            # no half is augmented
    with pytest.raises(ValueError, match="--shift_max 2000"):
        da.augmentation_factory(_args("--augment_past", "--augment_type", "pitch_wsola", "--shift_max", "2000"))


def test_checkpoint_args_keep_the_type(tmp_path):
    args = _args("--augment_past", "--augment_type", "pitch_wsola", "time_dropout", "--shift_max", "200")
    run = tmp_path / "run"
    run.mkdir()
    (run / "checkpoint_3.pt").write_bytes(b"")
    (run / "checkpoint_logs.json").write_text("{}")
    (run / "checkpoint_args.json").write_text(json.dumps(vars(args), indent=2))
    _path, _logs, kept = fl.getCheckpointData(str(run))
    assert kept.augment_type == ["pitch_wsola", "time_dropout"] and kept.shift_max == 200 and kept.augment_past is True
    resumed = argparse.Namespace(**vars(_args()))
    assert resumed.augment_type is None
    fl.loadArgs(resumed, kept)
    tr.refuseUnsupported(resumed)
    got = da.augmentation_factory(resumed)
    assert [type(t) for t in got.transfors_cfgs] == [da.PitchShiftAugment, da.TimeDropoutAugment]
    assert got.transfors_cfgs[0].shift_max == 200
