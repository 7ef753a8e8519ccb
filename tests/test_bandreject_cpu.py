"""The `bandreject_sinc` augmentation without a GPU: the draws of BandrejectSincAugment against the pairs the reference's
BandrejectAugment.generate_freq_mask returned (tests/golden/g30_bandreject_draws.json, tools/make_golden_bandreject.py), the host
tables of the definition, the frequency response of the numpy statement of tests/bandreject_oracle.py, the C entries' refusals and
the way from the command line to the transform."""
import argparse
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import bandreject_oracle as BO
from cpc2_amd import _lib
from cpc2_amd import data_augmentation as da
from cpc2_amd import feature_loader as fl
from cpc2_amd import train as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISSING = os.path.join(ROOT, "tests", "golden", "no_such_data_set")
with open(os.path.join(ROOT, "tests", "golden", "g30_bandreject_draws.json")) as _fh:
    GOLDEN = json.load(_fh)
CASES = GOLDEN["cases"]


# ----------------------------------------------------------------------------- the draws
def test_the_recorded_draws_seal_into_a_plan():
    assert GOLDEN["draws"] == 16 and {c["scaler"] for c in CASES} == {0.5, 1.0, 2.0}
    first, = [c for c in CASES if c["seed"] == 1234 and c["scaler"] == 1.0]
    assert tuple(first["pairs"][0]) == (2552.328389222971, 2722.165046087116)
    for c in CASES:                                                  # every recorded pair is a band the tables take as it is
        plan = da.BandrejectSincAugment(c["scaler"]).seal([tuple(p) for p in c["pairs"]], torch.device("cpu"))
        assert plan["band"].tolist() == c["pairs"] and plan["n"] == 16


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"seed{c['seed']}-scaler{c['scaler']}")
def test_draw_one_equals_the_references_draws(case):
    aug = da.BandrejectSincAugment(case["scaler"])
    np.random.seed(case["seed"])
    got = [aug.draw_one(20480) for _ in range(GOLDEN["draws"])]
    follows = np.random.uniform()
    assert [list(p) for p in got] == case["pairs"]
    assert all(type(v) is float for p in got for v in p)
    np.random.seed(case["seed"])
    for _ in range(GOLDEN["draws"]):                                 # exactly two uniforms per window: the generator is where it should be
        np.random.uniform(), np.random.uniform()
    assert follows == np.random.uniform()
    np.random.seed(case["seed"])
    assert [list(BO.draw(case["scaler"])) for _ in range(GOLDEN["draws"])] == case["pairs"]


def test_scaler_zero_draws_an_empty_band_and_bad_scalers_are_refused_by_name():
    aug = da.BandrejectSincAugment(0)
    np.random.seed(3)
    got = [aug.draw_one(64) for _ in range(50)]
    assert all(low == high for low, high in got) and len({low for low, _ in got}) == 50
    edge = da.BandrejectSincAugment(256 / 27)                        # the whole scale: still inside [0, 8000] once sealed
    np.random.seed(4)
    plan = edge.seal([edge.draw_one(64) for _ in range(50)], torch.device("cpu"))
    assert plan["low"].min() >= 0 and plan["high"].max() <= 8000 and (plan["low"] <= plan["high"]).all()
    for bad in (-0.01, 256 / 27 + 0.01, 10.0, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError) as err:
            da.BandrejectSincAugment(bad)
        assert str(err.value).startswith("scaler ")
        with pytest.raises(ValueError, match="^scaler "):
            da.get_augment("bandreject_sinc", bandreject_scaler=bad)
    for kwargs, name in (({"attenuation_dB": 50}, "attenuation_dB"), ({"attenuation_dB": 141}, "attenuation_dB"),
                         ({"attenuation_dB": float("nan")}, "attenuation_dB"), ({"transition_hz": 10.0}, "transition_hz"),
                         ({"transition_hz": 0.0}, "transition_hz"), ({"transition_hz": float("nan")}, "transition_hz")):
        with pytest.raises(ValueError) as err:
            da.BandrejectSincAugment(**kwargs)
        assert str(err.value).startswith(name + " "), err.value


# ----------------------------------------------------------------------------- the tables
def test_the_tables_are_the_definitions():
    t = da.bandreject_tables([100.0, 0.0], [200.0, 8000.0])
    assert (t["half"], t["taps"]) == (157, 315) and abs(t["beta"] - 12.26526) < 1e-12
    assert t["band"].dtype == np.float64 and t["band"].tolist() == [[100.0, 200.0], [0.0, 8000.0]]
    assert BO.design() == (t["beta"], 313, 157, 315)
    for (a, tbw), half in {(60, 400): 73, (80, 100): 402, (140, 400): 184, (120, 61.5): 1016}.items():
        got = da.bandreject_tables([1.0], [2.0], a, tbw)
        assert got["half"] == half == BO.design(a, tbw)[2] and got["taps"] == 2 * half + 1 and got["beta"] == BO.design(a, tbw)[0]
    empty = da.bandreject_tables([], [])
    assert empty["band"].shape == (0, 2) and empty["half"] == 157
    assert da.bandreject_tables([5.0], [5.0])["band"].tolist() == [[5.0, 5.0]]            # an empty band is a band


@pytest.mark.parametrize("kwargs,name", [
    (dict(transition_hz=60.0), "transition_hz"),                    # H = 1041
    (dict(transition_hz=1.0), "transition_hz"), (dict(transition_hz=1e-300), "transition_hz"),
    (dict(transition_hz=0.0), "transition_hz"), (dict(transition_hz=-400.0), "transition_hz"),
    (dict(transition_hz=float("nan")), "transition_hz"), (dict(transition_hz=float("inf")), "transition_hz"),
    (dict(attenuation_dB=50.0), "attenuation_dB"), (dict(attenuation_dB=140.5), "attenuation_dB"),
    (dict(attenuation_dB=float("nan")), "attenuation_dB"), (dict(attenuation_dB=float("inf")), "attenuation_dB"),
    (dict(low=[-1.0]), "low"), (dict(low=[float("nan")]), "low"), (dict(low=[float("inf")]), "low"), (dict(low=[300.0]), "low"),
    (dict(high=[8000.5]), "high"), (dict(high=[float("nan")]), "high"), (dict(high=[float("inf")]), "high"),
    (dict(high=[150.0, 160.0]), "high"),
], ids=lambda v: str(v))
def test_every_table_refusal_names_its_argument(kwargs, name):
    args = dict(low=[100.0], high=[200.0])
    args.update(kwargs)
    with pytest.raises(ValueError) as err:
        da.bandreject_tables(**args)
    assert str(err.value).startswith(name + " ") or str(err.value).startswith(name + ": "), err.value


def test_seal_builds_the_plan():
    aug = da.BandrejectSincAugment()
    plan = aug.seal([(100.0, 200.0), (0.0, 0.0), (7000.0, 8000.0)], torch.device("cpu"))
    assert plan["kind"] == "bandreject_sinc" and plan["n"] == 3 and plan["half"] == 157 and plan["taps"] == 315
    assert plan["low"].tolist() == [100.0, 0.0, 7000.0] and plan["high"].tolist() == [200.0, 0.0, 8000.0]
    assert plan["band"].shape == (3, 2) and plan["band"].dtype == np.float64
    assert plan["_dev"]["band"].dtype == torch.float64 and torch.equal(plan["_dev"]["band"], torch.from_numpy(plan["band"]))
    assert set(plan["_dev"]) == {"band"}                             # two doubles per window, no table of taps
    assert not aug.inplace
    assert da.BandrejectSincAugment(attenuation_dB=60).seal([(1.0, 2.0)], torch.device("cpu"))["half"] == 73


# ----------------------------------------------------------------------------- the definition itself
def test_the_statements_taps_reject_the_band_and_pass_the_rest():
    tables = da.bandreject_tables([1000.0], [2000.0])                # the filter the package's defaults specify
    beta, half, count = tables["beta"], tables["half"], tables["taps"]
    assert (beta, half, count) == (BO.design()[0], BO.design()[2], BO.design()[3])
    h = BO.taps(1000.0, 2000.0, half, beta)
    assert h.shape == (count,) and h.dtype == np.float64 and np.array_equal(h, h[::-1])
    stop = BO.response(h, np.linspace(1400, 1600, 2001))
    worst = 20 * np.log10(stop.max())
    ripple = np.abs(BO.response(h, np.concatenate([np.linspace(0, 600, 3001), np.linspace(2400, 8000, 20001)])) - 1).max()
    edges = BO.response(h, [1000.0, 2000.0])
    print(f"stop band {worst:.2f} dB, pass band ripple {ripple:.3e}, edges {edges}")
    assert worst <= -118
    assert ripple <= 1e-6
    assert np.abs(edges - 0.5).max() <= 1e-3
    for low, high in ((1500.0, 1500.0), (0.0, 0.0), (8000.0, 8000.0)):
        delta = BO.taps(low, high, half, beta)
        assert delta[half] == 1.0 and np.count_nonzero(delta) == 1 and delta.shape == (count,)
    x = np.random.RandomState(0).standard_normal((2, 700)).astype(np.float32)
    y = BO.bandreject(x, [300.0, 1000.0], [300.0, 2000.0], half, beta)
    assert np.array_equal(y[0], x[0].astype(np.float64)) and not np.array_equal(y[1], x[1].astype(np.float64))
    # the filter is the convolution with zeros outside the window: one sample by hand
    t = 5
    by_hand = sum(h[half + j] * float(x[1, t - j]) for j in range(-half, half + 1) if 0 <= t - j < 700)
    assert abs(y[1, t] - by_hand) <= 1e-13
    assert np.allclose(BO.reach(x, half)[1, t], np.abs(x[1, :t + half + 1].astype(np.float64)).sum(), rtol=1e-13)


# ----------------------------------------------------------------------------- the C entries
def test_abi_lists_the_entry_points_and_refuses_bad_arguments():
    for name in ("cpc_bandreject_tile", "cpc_bandreject_max_half", "cpc_bandreject_taps", "cpc_augment_bandreject"):
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.cpc_version() >= 127
    assert 64 <= lib.cpc_bandreject_tile() <= 8192 and lib.cpc_bandreject_max_half() == 1024 == da.BANDREJECT_MAX_HALF
    invalid = -1                                                     # CPC_ERR_INVALID
    # host buffers that a refused call never touches (nothing is launched: no device is needed)
    src = (ctypes.c_float * 16)()
    out = (ctypes.c_float * 16)(*([7.0] * 16))
    band = (ctypes.c_double * 2)(100.0, 200.0)
    taps = (ctypes.c_double * 8)(*([7.0] * 8))
    S, O, B, T = (ctypes.cast(v, ctypes.c_void_p) for v in (src, out, band, taps))
    nan, inf = float("nan"), float("inf")

    def filt(src=S, total=0, off=None, band=B, half=3, beta=12.0, sr=16000.0, out=O, batch=1, window=16):
        return lib.cpc_augment_bandreject(src, total, off, band, half, beta, sr, out, batch, window, None)

    def design(band=B, batch=1, half=3, beta=12.0, sr=16000.0, taps=T):
        return lib.cpc_bandreject_taps(band, batch, half, beta, sr, taps, None)

    shared = {"batch -1": dict(batch=-1), "batch 65536": dict(batch=65536), "half 0": dict(half=0), "half -1": dict(half=-1),
              "half 1025": dict(half=1025), "beta nan": dict(beta=nan), "beta inf": dict(beta=inf), "beta < 0": dict(beta=-0.5),
              "beta > 50": dict(beta=50.5), "rate 0": dict(sr=0.0), "rate < 0": dict(sr=-16000.0), "rate nan": dict(sr=nan),
              "rate inf": dict(sr=inf), "band null": dict(band=None)}
    only_filter = {"window 0": dict(window=0), "window -1": dict(window=-1), "src null": dict(src=None), "out null": dict(out=None),
                   "out == src": dict(out=S), "offsets without a length": dict(off=B, total=0)}
    for what, kwargs in {**shared, **only_filter}.items():
        assert filt(**kwargs) == invalid, what
        assert lib.cpc_last_error().startswith(b"augment_bandreject:"), (what, lib.cpc_last_error())
    for what, kwargs in {**shared, "taps null": dict(taps=None)}.items():
        assert design(**kwargs) == invalid, what
        assert lib.cpc_last_error().startswith(b"bandreject_taps:"), (what, lib.cpc_last_error())
    assert list(out) == [7.0] * 16 and list(taps) == [7.0] * 8 and list(src) == [0.0] * 16
    assert filt(batch=0) == 0 and filt(batch=0, src=None, band=None, out=None) == 0          # a no-op
    assert design(batch=0) == 0 and design(batch=0, band=None, taps=None) == 0
    assert list(out) == [7.0] * 16 and list(taps) == [7.0] * 8


# ----------------------------------------------------------------------------- from the command line to the transform
def _args(*flags):
    args = tr.parseArgs(["--pathDB", MISSING, "--nGPU", "0", "--random_seed", "0"] + list(flags))
    args.nGPU = 1                                       # (parseArgs checks --nGPU against the devices present; the factory multiplies by it)
    return args


def test_the_lists_of_types():
    from cpc2_amd.cpc_default_config import AUGMENT_TYPES
    assert da.FILTER_TYPES == ("bandreject_sinc",)
    assert da.BUILT_TYPES == ("additive", "natural_reverb", "time_dropout", "pitch_wsola") and da.OWN_TYPES == ("freeverb",)
    assert "bandreject_sinc" in AUGMENT_TYPES and "bandreject" in AUGMENT_TYPES
    assert {"bandreject", "random_noise"} <= set(da.UNBUILT_TYPES) and "bandreject_sinc" not in da.UNBUILT_TYPES
    message = da.unbuilt_message(["bandreject_sinc", "bandreject"])
    assert ": bandreject is not built" in message
    assert "additive, natural_reverb, time_dropout, pitch_wsola, freeverb and none" in message
    assert "are bandreject_sinc, additive" in message                # named as built, outside the pinned substring


@pytest.mark.parametrize("flags", [
    ["--augment_past", "--augment_type", "bandreject_sinc"],
    ["--augment_past", "--augment_type", "bandreject_sinc", "time_dropout"],
    ["--augment_future", "--augment_type", "additive", "bandreject_sinc", "--pathDBNoise", "noise"],
], ids=" ".join)
def test_refuse_unsupported_lets_bandreject_sinc_through(flags):
    tr.refuseUnsupported(_args(*flags))


def test_the_sox_name_stays_refused():
    for flags in (["--augment_type", "bandreject"], ["--augment_type", "bandreject_sinc", "bandreject"]):
        args = _args("--augment_past", *flags)
        with pytest.raises(NotImplementedError, match="bandreject") as err:
            tr.refuseUnsupported(args)
        assert ": bandreject is not built" in str(err.value)                      # bandreject_sinc is not among the missing
        assert "are bandreject_sinc, additive, natural_reverb, time_dropout, pitch_wsola, freeverb and none" in str(err.value)
        with pytest.raises(NotImplementedError, match="bandreject"):
            da.augmentation_factory(args)
    with pytest.raises(NotImplementedError, match="bandreject"):
        da.get_augment("bandreject")
    with pytest.raises(SystemExit):                                  # --meta_aug_type is not extended
        _args("--meta_aug", "--meta_aug_type", "bandreject_sinc")


def test_the_factory_builds_the_transform_and_its_combinations():
    got = da.augmentation_factory(_args("--augment_past", "--augment_type", "bandreject_sinc"))
    assert type(got) is da.BandrejectSincAugment and not got.inplace
    assert (got.scaler, got.attenuation_dB, got.transition_hz) == (1.0, 120.0, 400.0)
    got = da.augmentation_factory(_args("--augment_past", "--augment_type", "bandreject_sinc", "--bandreject_scaler", "0.5"))
    assert type(got) is da.BandrejectSincAugment and got.scaler == 0.5
    np.random.seed(7)
    case, = [c for c in CASES if c["seed"] == 7 and c["scaler"] == 0.5]
    assert list(got.draw_one(20480)) == case["pairs"][0]
    got = da.augmentation_factory(_args("--augment_future", "--augment_type", "bandreject_sinc", "time_dropout", "freeverb", "--t_ms",
                                        "20", "--bandreject_scaler", "2"))
    assert type(got) is da.CombinedTransforms
    assert [type(t) for t in got.transfors_cfgs] == [da.BandrejectSincAugment, da.TimeDropoutAugment, da.FreeverbAugment]
    assert got.transfors_cfgs[0].scaler == 2.0 and got.transfors_cfgs[1].max_frames == 320
    # the parts draw in their order, window by window
    np.random.seed(13)
    entries = [got.draw_one(4096) for _ in range(5)]
    np.random.seed(13)
    for entry in entries:
        band = BO.draw(2.0)
        length = int(np.random.randint(0, 320))
        drop = (int(np.random.randint(0, max(1, 4096 - length))), length)
        assert entry == (band, drop, int(np.random.randint(0, 100)))
    plan = got.seal(entries, torch.device("cpu"))
    assert [p["kind"] for p in plan["parts"]] == ["bandreject_sinc", "time_dropout", "freeverb"]
    assert plan["parts"][0]["low"].tolist() == [e[0][0] for e in entries]
    assert da.augmentation_factory(_args("--augment_type", "bandreject_sinc")) is None         # no half is augmented
    assert type(da.get_augment("bandreject_sinc")) is da.BandrejectSincAugment and da.get_augment("bandreject_sinc").scaler == 1.0
    with pytest.raises(ValueError, match="^scaler "):
        da.augmentation_factory(_args("--augment_past", "--augment_type", "bandreject_sinc", "--bandreject_scaler", "10"))


def test_checkpoint_args_keep_the_type(tmp_path):
    args = _args("--augment_past", "--augment_type", "bandreject_sinc", "time_dropout", "--bandreject_scaler", "0.5")
    run = tmp_path / "run"
    run.mkdir()
    (run / "checkpoint_3.pt").write_bytes(b"")
    (run / "checkpoint_logs.json").write_text("{}")
    (run / "checkpoint_args.json").write_text(json.dumps(vars(args), indent=2))
    _path, _logs, kept = fl.getCheckpointData(str(run))
    assert kept.augment_type == ["bandreject_sinc", "time_dropout"] and kept.augment_past is True and kept.bandreject_scaler == 0.5
    resumed = argparse.Namespace(**vars(_args()))
    assert resumed.augment_type is None
    fl.loadArgs(resumed, kept)
    assert resumed.augment_type == ["bandreject_sinc", "time_dropout"]
    tr.refuseUnsupported(resumed)
    got = da.augmentation_factory(resumed)
    assert [type(t) for t in got.transfors_cfgs] == [da.BandrejectSincAugment, da.TimeDropoutAugment]
    assert got.transfors_cfgs[0].scaler == 0.5


def test_no_cpu_fallback():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        da.BandrejectSincAugment()(torch.zeros(2, 1, 64))
    from cpc2_amd import audio
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        audio.bandreject(torch.zeros(2, 64), 100.0, 200.0)
