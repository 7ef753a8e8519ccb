"""The `freeverb` augmentation without a GPU: the host tables of the definition (delay lengths, feedback, damping), the draws of
FreeverbAugment (the reference's one np.random.randint(0, room_max) per window), the constructor's and the C entry's refusals, the
way from the command line to the transform, and two sanity checks of the numpy statement of tests/freeverb_oracle.py."""
import argparse
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import augment_oracle as AO
import freeverb_oracle as FO
from cpc2_amd import _lib
from cpc2_amd import data_augmentation as da
from cpc2_amd import dataset as ds
from cpc2_amd import feature_loader as fl
from cpc2_amd import train as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISSING = os.path.join(ROOT, "tests", "golden", "no_such_data_set")

D_ROWS = {0: (40, 43, 46, 49, 52, 54, 56, 59),
          99: (401, 427, 459, 488, 511, 536, 560, 581),
          50: (223, 237, 255, 271, 284, 298, 311, 323)}
A_ROW = (82, 124, 160, 202)
FB_50 = 0.8816784043380077


# ----------------------------------------------------------------------------- the tables
def test_the_tables_are_the_definitions():
    t = da.freeverb_tables([0, 99, 50])
    assert t["room"].dtype == np.int32 and t["room"].tolist() == [0, 99, 50]
    assert t["comb_len"].dtype == np.int32 and t["comb_len"].shape == (3, 8)
    for row, rs in enumerate((0, 99, 50)):
        assert tuple(t["comb_len"][row].tolist()) == D_ROWS[rs] == FO.comb_lengths(rs)
    assert tuple(t["allpass_len"]) == A_ROW == FO.allpass_lengths()
    assert t["len_bound"] == 581
    assert abs(t["feedback64"] - 0.98) <= 1e-15 and t["feedback"] == float(np.float32(0.98))
    assert t["damping"] == 0.5 and t["gain"] == float(np.float32(0.015))
    half = da.freeverb_tables([7], 50.0, 50.0)
    assert abs(half["feedback64"] - FB_50) <= 1e-15 and half["feedback"] == float(np.float32(FB_50))
    assert half["damping"] == float(np.float32(0.35)) and abs(FO.scalars(50.0, 50.0)[1] - 0.35) <= 1e-15
    assert abs(FO.scalars()[0] - 0.98) <= 1e-15 and abs(FO.scalars(50.0, 50.0)[0] - FB_50) <= 1e-15
    assert da.freeverb_tables([3], wet_gain_dB=-20.0)["gain"] == float(np.float32(0.0015))
    # every room of the definition: the package's table is the statement's, and the lengths grow with the room
    rooms = np.arange(100)
    table = da.freeverb_tables(rooms)["comb_len"]
    assert table.tolist() == [list(FO.comb_lengths(int(r))) for r in rooms]
    assert (np.diff(table, axis=0) >= 0).all() and (np.diff(table, axis=1) > 0).all() and table.min() == 40
    empty = da.freeverb_tables([])
    assert empty["comb_len"].shape == (0, 8) and empty["len_bound"] == 1
    for bad in ([-1], [101]):
        with pytest.raises(ValueError, match="room size"):
            da.freeverb_tables(bad)


def test_seal_builds_the_plan():
    aug = da.FreeverbAugment()
    plan = aug.seal([0, 99, 50, 1], torch.device("cpu"))
    assert plan["kind"] == "freeverb" and plan["n"] == 4 and plan["len_bound"] == 581
    assert plan["room"].tolist() == [0, 99, 50, 1] and tuple(plan["allpass_len"]) == A_ROW
    assert plan["comb_len"].shape == (4, 8) and tuple(plan["comb_len"][1].tolist()) == D_ROWS[99]
    assert plan["_dev"]["comb_len"].dtype == torch.int32 and torch.equal(plan["_dev"]["comb_len"], torch.from_numpy(plan["comb_len"]))
    assert {"feedback", "damping", "gain"} <= set(plan) and plan["feedback"] == float(np.float32(0.98)) and plan["damping"] == 0.5
    assert not aug.inplace
    plan = da.FreeverbAugment(reverberance=50, hf_damping=50).seal([5], torch.device("cpu"))
    assert plan["feedback"] == float(np.float32(FB_50)) and plan["damping"] == float(np.float32(0.35))


# ----------------------------------------------------------------------------- the draws
def test_one_randint_per_window():
    aug = da.FreeverbAugment()
    np.random.seed(21)
    got = [aug.draw_one(20480) for _ in range(300)]
    follows = np.random.randint(0, 1 << 30)
    np.random.seed(21)
    assert got == [int(np.random.randint(0, 100)) for _ in range(300)]
    assert follows == np.random.randint(0, 1 << 30)                  # exactly one draw per window: the generator is where it should be
    assert min(got) == 0 and max(got) == 99
    aug = da.FreeverbAugment(room_max=3.0)
    np.random.seed(22)
    got = [aug.draw_one(64) for _ in range(100)]
    np.random.seed(22)
    assert got == [int(np.random.randint(0, 3)) for _ in range(100)] and set(got) == {0, 1, 2}


@pytest.mark.parametrize("order", [["freeverb", "time_dropout"], ["time_dropout", "none", "freeverb"],
                                   ["pitch_wsola", "freeverb", "time_dropout"]], ids="+".join)
def test_combined_transforms_draw_in_the_order_of_the_parts(order):
    w = 20480
    aug = da.CombinedTransforms(order, shift_max=250, t_ms=100)
    names = {"freeverb": "FreeverbAugment", "time_dropout": "TimeDropoutAugment", "pitch_wsola": "PitchShiftAugment"}
    assert [type(t).__name__ for t in aug._parts] == [names[t] for t in order if t != "none"]
    np.random.seed(13)
    got = [aug.draw_one(w) for _ in range(20)]
    np.random.seed(13)
    for entry in got:
        want = []
        for t in order:
            if t == "freeverb":
                want.append(int(np.random.randint(0, 100)))
            elif t == "pitch_wsola":
                want.append(int(np.random.randint(-250, 250)))
            elif t == "time_dropout":
                length = int(np.random.randint(0, 1600))
                want.append((int(np.random.randint(0, max(1, w - length))), length))
        assert entry == tuple(want)
    plan = aug.seal(got, torch.device("cpu"))
    kinds = [p["kind"] for p in plan["parts"]]
    assert kinds == [t for t in order if t != "none"]
    part = plan["parts"][kinds.index("freeverb")]
    assert part["room"].tolist() == [e[kinds.index("freeverb")] for e in got]


# ----------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("kwargs,name", [
    ({"room_max": 0}, "room_max"), ({"room_max": 101}, "room_max"), ({"room_max": 2.5}, "room_max"), ({"room_max": -3}, "room_max"),
    ({"room_max": float("nan")}, "room_max"), ({"room_max": float("inf")}, "room_max"),
    ({"reverberance": -0.1}, "reverberance"), ({"reverberance": 100.5}, "reverberance"),
    ({"reverberance": float("nan")}, "reverberance"),
    ({"hf_damping": -1}, "hf_damping"), ({"hf_damping": 101}, "hf_damping"), ({"hf_damping": float("nan")}, "hf_damping"),
    ({"wet_gain_dB": float("inf")}, "wet_gain_dB"), ({"wet_gain_dB": float("-inf")}, "wet_gain_dB"),
    ({"wet_gain_dB": float("nan")}, "wet_gain_dB"), ({"wet_gain_dB": 900.0}, "wet_gain_dB"),
], ids=lambda v: str(v))
def test_every_constructor_refusal_names_its_argument(kwargs, name):
    with pytest.raises(ValueError) as err:
        da.FreeverbAugment(**kwargs)
    assert str(err.value).startswith(name + " ")
    ok = da.FreeverbAugment(room_max=1, reverberance=0, hf_damping=0, wet_gain_dB=-60.0)
    assert ok.room_max == 1 and ok.draw_one(8) == 0


def test_abi_lists_the_entry_point_and_refuses_bad_arguments():
    assert "cpc_augment_freeverb" in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.cpc_version() >= 125
    invalid = -1                                                     # CPC_ERR_INVALID
    # host buffers that a refused call never touches (nothing is launched: no device is needed)
    src = (ctypes.c_float * 16)()
    out = (ctypes.c_float * 16)(*([7.0] * 16))
    table = (ctypes.c_int * 8)(*D_ROWS[0])
    S, O, T = (ctypes.cast(v, ctypes.c_void_p) for v in (src, out, table))
    good_ap = (ctypes.c_int * 4)(*A_ROW)

    def call(src=S, total=0, off=None, table=T, bound=59, ap=good_ap, fb=0.98, dmp=0.5, g=0.015, out=O, batch=1, window=16):
        return lib.cpc_augment_freeverb(src, total, off, table, bound, ap, fb, dmp, g, out, batch, window, None)

    nan, inf = float("nan"), float("inf")
    cases = {"window 0": dict(window=0), "window -1": dict(window=-1), "batch -1": dict(batch=-1), "batch 65536": dict(batch=65536),
             "len_bound 0": dict(bound=0), "len_bound 1025": dict(bound=1025),
             "allpass 0": dict(ap=(ctypes.c_int * 4)(82, 0, 160, 202)), "allpass 1025": dict(ap=(ctypes.c_int * 4)(82, 124, 160, 1025)),
             "allpass null": dict(ap=None),
             "feedback 1": dict(fb=1.0), "feedback < 0": dict(fb=-0.01), "feedback nan": dict(fb=nan), "feedback inf": dict(fb=inf),
             "damping > 1": dict(dmp=1.01), "damping < 0": dict(dmp=-0.01), "damping nan": dict(dmp=nan),
             "gain nan": dict(g=nan), "gain inf": dict(g=inf), "gain -inf": dict(g=-inf),
             "src null": dict(src=None), "table null": dict(table=None), "out null": dict(out=None), "out == src": dict(out=S),
             "offsets without a length": dict(off=T, total=0)}
    for what, kwargs in cases.items():
        assert call(**kwargs) == invalid, what
        assert lib.cpc_last_error().startswith(b"augment_freeverb:"), what
    assert list(out) == [7.0] * 16
    assert call(batch=0) == 0 and call(batch=0, src=None, table=None, out=None) == 0          # a no-op
    assert list(out) == [7.0] * 16


# ----------------------------------------------------------------------------- from the command line to the transform
def _args(*flags):
    args = tr.parseArgs(["--pathDB", MISSING, "--nGPU", "0", "--random_seed", "0"] + list(flags))
    args.nGPU = 1                                       # (parseArgs checks --nGPU against the devices present; the factory multiplies by it)
    return args


@pytest.mark.parametrize("flags", [
    ["--augment_past", "--augment_type", "freeverb"],
    ["--augment_past", "--augment_type", "freeverb", "time_dropout"],
    ["--augment_future", "--augment_type", "additive", "freeverb", "--pathDBNoise", "noise"],
    ["--augment_past", "--augment_type", "pitch_wsola", "freeverb", "none"],
], ids=" ".join)
def test_refuse_unsupported_lets_freeverb_through(flags):
    tr.refuseUnsupported(_args(*flags))


@pytest.mark.parametrize("unbuilt", ["artificial_reverb", "artificial_reverb_dropout", "bandreject"])
def test_the_sox_names_stay_refused(unbuilt):
    for flags in (["--augment_type", unbuilt], ["--augment_type", "freeverb", unbuilt]):
        args = _args("--augment_past", *flags)
        with pytest.raises(NotImplementedError, match=unbuilt) as err:
            tr.refuseUnsupported(args)
        assert "additive, natural_reverb, time_dropout, pitch_wsola, freeverb and none" in str(err.value)
        assert f": {unbuilt} is not built" in str(err.value)                      # freeverb is not among the missing
        with pytest.raises(NotImplementedError, match=unbuilt):
            da.augmentation_factory(args)
    with pytest.raises(NotImplementedError, match=unbuilt):
        da.get_augment(unbuilt)


def test_the_lists_of_types():
    from cpc2_amd.cpc_default_config import AUGMENT_TYPES
    assert da.OWN_TYPES == ("freeverb",) and "freeverb" not in da.BUILT_TYPES and "freeverb" not in da.UNBUILT_TYPES
    assert "freeverb" in AUGMENT_TYPES
    assert {"artificial_reverb", "artificial_reverb_dropout", "bandreject", "random_noise"} <= set(da.UNBUILT_TYPES)
    message = da.unbuilt_message(["freeverb", "artificial_reverb"])
    assert "artificial_reverb is not built" in message
    assert "additive, natural_reverb, time_dropout, pitch_wsola, freeverb and none" in message


def test_the_factory_builds_the_transform_and_its_combinations(tmp_path, capsys):
    got = da.augmentation_factory(_args("--augment_past", "--augment_type", "freeverb"))
    assert type(got) is da.FreeverbAugment and not got.inplace
    assert (got.room_max, got.reverberance, got.hf_damping, got.wet_gain_dB) == (100, 100.0, 100.0, 0.0)
    got = da.augmentation_factory(_args("--augment_future", "--augment_type", "freeverb", "time_dropout", "--t_ms", "20"))
    assert type(got) is da.CombinedTransforms
    assert [type(t) for t in got.transfors_cfgs] == [da.FreeverbAugment, da.TimeDropoutAugment]
    assert got.transfors_cfgs[1].max_frames == 320
    noise_db = AO.make_noise_db(tmp_path / "noise")
    seqs, _ = ds.findAllSeqs(noise_db, extension=".wav", speaker_level=0)
    noise = ds.AudioBatchData(noise_db, 2048, seqs, None, 1, transform=ds.PeakNorm(), keep_temporality=False, device="cpu")
    got = da.augmentation_factory(_args("--augment_past", "--augment_type", "additive", "freeverb", "--pathDBNoise", noise_db), noise)
    assert [type(t) for t in got.transfors_cfgs] == [da.AdditiveNoiseAugment, da.FreeverbAugment]
    assert da.augmentation_factory(_args("--augment_type", "freeverb")) is None                # no half is augmented
    # the reverberated noise: --meta_aug_type freeverb
    args = _args("--augment_past", "--augment_type", "additive", "--pathDBNoise", noise_db, "--meta_aug", "--meta_aug_type", "freeverb")
    assert type(da.augmentation_factory(args, applied_on_noise=True)) is da.FreeverbAugment
    assert type(da.get_augment("freeverb")) is da.FreeverbAugment


def test_checkpoint_args_keep_the_type(tmp_path):
    args = _args("--augment_past", "--augment_type", "freeverb", "time_dropout")
    run = tmp_path / "run"
    run.mkdir()
    (run / "checkpoint_3.pt").write_bytes(b"")
    (run / "checkpoint_logs.json").write_text("{}")
    (run / "checkpoint_args.json").write_text(json.dumps(vars(args), indent=2))
    _path, _logs, kept = fl.getCheckpointData(str(run))
    assert kept.augment_type == ["freeverb", "time_dropout"] and kept.augment_past is True
    resumed = argparse.Namespace(**vars(_args()))
    assert resumed.augment_type is None
    fl.loadArgs(resumed, kept)
    assert resumed.augment_type == ["freeverb", "time_dropout"]
    tr.refuseUnsupported(resumed)
    got = da.augmentation_factory(resumed)
    assert [type(t) for t in got.transfors_cfgs] == [da.FreeverbAugment, da.TimeDropoutAugment]


# ----------------------------------------------------------------------------- the statement
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("w", [1, 39, 40])
def test_a_window_no_longer_than_the_shortest_line_comes_back(w, dtype):
    x = (0.1 * np.random.RandomState(w).standard_normal((2, w))).astype(np.float32)
    y = FO.freeverb(x, [0, 0], dtype=dtype)
    assert y.dtype == dtype and np.array_equal(y, x.astype(dtype))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_a_unit_impulse_meets_the_first_comb_at_its_length(dtype):
    rooms = [0, 1, 50, 98, 99]
    x = np.zeros((len(rooms), 700), dtype=np.float32)
    x[:, 0] = 1.0
    y = FO.freeverb(x, rooms, dtype=dtype)
    for row, rs in enumerate(rooms):
        first = FO.comb_lengths(rs)[0]
        assert y[row, 0] == 1.0 and not y[row, 1:first].any()
        assert y[row, first] == dtype(np.float32(0.015)), (rs, first)          # g itself: through four empty all-passes, sign + + + +
    # and the two evaluations differ by rounding alone
    both = FO.freeverb(x, rooms, dtype=np.float32).astype(np.float64) - FO.freeverb(x, rooms, dtype=np.float64)
    assert np.abs(both).max() < 1e-7


def test_the_tail_decays_and_damping_shortens_it():
    x = np.zeros((1, 8000), dtype=np.float32)
    x[0, 0] = 1.0
    long = FO.freeverb(x, [50])[0]
    short = FO.freeverb(x, [50], 50.0, 50.0)[0]
    late = slice(6000, 8000)
    assert np.isfinite(long).all() and np.abs(long[late]).max() < np.abs(long[300:2300]).max()
    assert np.sqrt(np.mean(short[late] ** 2)) < 0.2 * np.sqrt(np.mean(long[late] ** 2))


def test_no_cpu_fallback():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        da.FreeverbAugment()(torch.zeros(2, 1, 64))
    from cpc2_amd import audio
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        audio.freeverb(torch.zeros(2, 64), 5)
