#!/usr/bin/env python3
"""Generate tests/golden/g24_augment.npz and tests/golden/g24_augment_factory.json by running the REFERENCE's augmentation code
on the CPU.

Needs a checkout of the reference repository (the directory that holds its `cpc` package); run from the repository root:
    CPC_REFERENCE=DIR PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_augment.py

The reference is imported unmodified; torchaudio, augment, torch_audiomentations, progressbar and psutil are registered as
stand-in modules, as tools/make_golden_train_cli.py does.  Two of the stand-ins carry a little behaviour here, so that the
reference's constructors run: `augment.effects.EffectChain` accepts any chain of calls, and
`torch_audiomentations.ApplyImpulseResponse` lists the .wav files it is given.  Neither is ever applied to audio.

g24_augment.npz (data only):
  * `add{i}_x`, `add{i}_noise`, `add{i}_seed`, `add{i}_snr` (min, max), `add{i}_out`: AdditiveNoiseAugment.__call__ on one
    [1, W] window after np.random.seed(seed), the noise window coming from a stand-in noise data set (the reference takes
    `next(loader)[0][0, 0]`); among them an all-zero noise window and an all-zero speech window;
  * `pn_in` / `pn_out` (PeakNorm), `en_in` / `en_out` (energy_normalization), `pk_in` / `pk_out` (peak_normalization).

g24_augment_factory.json: what augmentation_factory returns for a table of argument sets -- the class name (and the classes
inside a CombinedTransforms, and NaturalReverb's batch_wise), None, or the error -- for both applied_on_noise values, single and
combined types.  `$IR` stands for a directory that holds one .wav impulse response."""
import contextlib
import io
import json
import os
import sys
import tempfile
import types
import wave

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("CPC_REFERENCE")
if not REF or not os.path.isdir(os.path.join(REF, "cpc")):
    raise SystemExit("set CPC_REFERENCE to a checkout of the reference repository (the directory that holds cpc/)")
OUT_NPZ = os.path.join(ROOT, "tests", "golden", "g24_augment.npz")
OUT_JSON = os.path.join(ROOT, "tests", "golden", "g24_augment_factory.json")
for name in ("torchaudio", "augment", "augment.effects", "torch_audiomentations", "progressbar", "psutil"):
    sys.modules[name] = types.ModuleType(name)
sys.modules["augment"].effects = sys.modules["augment.effects"]


class _Chain:
    """Stand-in for augment.effects.EffectChain: any effect can be chained, none is ever applied."""

    def __getattr__(self, _name):
        return lambda *a, **k: self


class _ImpulseResponses:
    """Stand-in for torch_audiomentations.ApplyImpulseResponse: remembers the files, is never applied."""

    def __init__(self, ir_paths, p, sample_rate):
        if isinstance(ir_paths, str):
            ir_paths = sorted(os.path.join(r, f) for r, _d, fs in os.walk(ir_paths) for f in fs if f.endswith(".wav"))
        self.ir_paths, self.p, self.sample_rate = list(ir_paths), p, sample_rate


sys.modules["augment.effects"].EffectChain = _Chain
for name in ("Compose", "AddBackgroundNoise"):
    setattr(sys.modules["torch_audiomentations"], name, None)
sys.modules["torch_audiomentations"].ApplyImpulseResponse = _ImpulseResponses
sys.path.insert(0, REF)
os.chdir(ROOT)
import cpc.data_augmentation as ref_aug  # noqa: E402
import cpc.dataset as ref_ds  # noqa: E402


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


class NoiseStandIn:
    """What AdditiveNoiseAugment needs of a noise data set: getDataLoader(...) -> batches ([b, 2, 1, W], label)."""

    def __init__(self, windows):
        self.windows = windows          # [n, W]

    def getDataLoader(self, batchSize, **_k):
        n, w = self.windows.shape
        batch = self.windows.view(n, 1, 1, w).expand(n, 2, 1, w)
        return [(batch, torch.zeros(n, dtype=torch.long))]


# ----------------------------------------------------------------------------- arithmetic
def record_arithmetic():
    gen = torch.Generator().manual_seed(24)
    w = 1024
    out = {}
    cases = [("plain", 3, (5.0, 20.0)), ("loud_noise", 4, (-5.0, 0.0)), ("fixed_snr", 5, (10.0, 10.0)), ("zero_noise", 6, (5.0, 20.0)),
             ("zero_speech", 7, (5.0, 20.0)), ("tiny", 8, (0.0, 30.0))]
    for i, (tag, seed, (lo, hi)) in enumerate(cases):
        x = torch.randn(1, w, generator=gen) * 0.1 * torch.linspace(0.2, 1.0, w)
        noise = torch.rand(1, w, generator=gen) - 0.5
        if tag == "zero_noise":
            noise = torch.zeros(1, w)
        if tag == "zero_speech":
            x = torch.zeros(1, w)
        if tag == "tiny":
            x, noise = x * 1e-6, noise * 1e-7
        aug = ref_aug.AdditiveNoiseAugment(NoiseStandIn(noise), lo, hi, 1, "uniform")
        np.random.seed(seed)
        y = aug(x)
        out[f"add{i}_x"], out[f"add{i}_noise"] = x.numpy(), noise.numpy()
        out[f"add{i}_seed"], out[f"add{i}_snr"] = np.int64(seed), np.array([lo, hi], dtype=np.float64)
        out[f"add{i}_out"] = y.numpy()
        assert y.shape == (1, w) and y.dtype == torch.float32
    out["add_count"] = np.int64(len(cases))
    z = torch.randn(3, 512, generator=gen) * torch.tensor([[1.0], [1e-3], [0.0]])
    out["pn_in"], out["pn_out"] = z.numpy(), ref_ds.PeakNorm()(z).numpy()
    out["pk_in"], out["pk_out"] = z.numpy(), ref_aug.peak_normalization(z).numpy()
    e = torch.randn(1, 512, generator=gen) * 0.3
    out["en_in"], out["en_out"] = e.numpy(), ref_aug.energy_normalization(e).numpy()
    out["en_zero_out"] = ref_aug.energy_normalization(torch.zeros(1, 512)).numpy()
    return out


# ----------------------------------------------------------------------------- the factory's dispatch
BASE = dict(augment_past=True, augment_future=False, augment_type=None, meta_aug_type=None, ir_batch_wise=False,
            meta_ir_batch_wise=False, nGPU=1, batchSizeGPU=4, temporal_additive_noise=False, bandreject_scaler=1.0, t_ms=100,
            min_snr_in_db=5.0, max_snr_in_db=20.0, impulse_response_prob=1.0, pathImpulseResponses="$IR", ir_sample_rate=16000,
            shift_max=300)
TABLE = [
    ("nothing_augmented", dict(augment_past=False, augment_type=["additive"]), True, False),
    ("future_only_additive", dict(augment_past=False, augment_future=True, augment_type=["additive"]), True, False),
    ("no_type", dict(), True, False),
    ("type_none", dict(augment_type=["none"]), True, False),
    ("additive", dict(augment_type=["additive"]), True, False),
    ("additive_temporal", dict(augment_type=["additive"], temporal_additive_noise=True), True, False),
    ("additive_without_noise", dict(augment_type=["additive"]), False, False),
    ("natural_reverb", dict(augment_type=["natural_reverb"]), False, False),
    ("natural_reverb_batch_wise", dict(augment_type=["natural_reverb"], ir_batch_wise=True), False, False),
    ("time_dropout", dict(augment_type=["time_dropout"], t_ms=50), False, False),
    ("additive_reverb", dict(augment_type=["additive", "natural_reverb"]), True, False),
    ("reverb_additive_dropout", dict(augment_type=["natural_reverb", "additive", "time_dropout"]), True, False),
    ("none_inside", dict(augment_type=["none", "time_dropout"]), False, False),
    ("combined_without_noise", dict(augment_type=["additive", "natural_reverb"]), False, False),
    ("pitch", dict(augment_type=["pitch"]), False, False),
    ("bandreject", dict(augment_type=["bandreject"]), False, False),
    ("artificial_reverb", dict(augment_type=["artificial_reverb"]), False, False),
    ("artificial_reverb_dropout", dict(augment_type=["artificial_reverb_dropout"]), False, False),
    ("additive_bandreject", dict(augment_type=["additive", "bandreject"]), True, False),
    ("meta_off", dict(augment_type=["additive"]), False, True),
    ("meta_reverb", dict(augment_type=["additive"], meta_aug_type=["natural_reverb"]), False, True),
    ("meta_reverb_batch_wise", dict(augment_type=["additive"], meta_aug_type=["natural_reverb"], meta_ir_batch_wise=True,
                                    ir_batch_wise=False), False, True),
    ("meta_reverb_speech_batch_wise", dict(augment_type=["additive"], meta_aug_type=["natural_reverb"], ir_batch_wise=True), False,
     True),
    ("meta_nothing_augmented", dict(augment_past=False, augment_type=["additive"], meta_aug_type=["natural_reverb"]), False, True),
]


def write_wav(path, samples, rate=16000):
    with wave.open(path, "wb") as fh:
        fh.setnchannels(1)
        fh.setsampwidth(2)
        fh.setframerate(rate)
        fh.writeframes((np.clip(samples, -1, 1) * 32767).astype("<i2").tobytes())


def describe(obj):
    if obj is None:
        return {"class": None}
    out = {"class": type(obj).__name__}
    if isinstance(obj, ref_aug.CombinedTransforms):
        out["parts"] = [None if t is None else type(t).__name__ for t in obj.transfors_cfgs]
    if isinstance(obj, ref_aug.NaturalReverb):
        out["batch_wise"] = bool(obj.batch_wise)
    if isinstance(obj, ref_aug.AdditiveNoiseAugment):
        out["sampling"] = obj.sampling
        out["batchSize"] = obj.batchSize
    return out


def record_factory():
    ir_dir = tempfile.mkdtemp(prefix="g24_ir_")
    write_wav(os.path.join(ir_dir, "room.wav"), np.exp(-np.arange(64) / 8.0) * 0.5)
    noise = NoiseStandIn(torch.zeros(4, 64))
    out = {}
    for tag, changes, with_noise, on_noise in TABLE:
        values = dict(BASE, **changes)
        args = types.SimpleNamespace(**dict(values, pathImpulseResponses=ir_dir))
        try:
            result = describe(quiet(ref_aug.augmentation_factory, args, noise if with_noise else None, applied_on_noise=on_noise))
        except Exception as err:                                    # noqa: BLE001 -- the error IS the recorded result
            result = {"error": type(err).__name__, "message": str(err)}
        out[tag] = {"args": values, "noise_dataset": with_noise, "applied_on_noise": on_noise, "result": result}
    return out


def main():
    np.savez_compressed(OUT_NPZ, **record_arithmetic())
    with open(OUT_JSON, "w") as fh:
        json.dump(record_factory(), fh, indent=1, sort_keys=True)
    for path in (OUT_NPZ, OUT_JSON):
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
