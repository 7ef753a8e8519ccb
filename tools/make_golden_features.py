#!/usr/bin/env python3
"""Generate tests/golden/g25_features.npz, g25_features_wide.npz and g25_features.json by running the REFERENCE's feature
extraction (cpc/feature_loader.py: buildFeature, buildFeature_batch, seqNormalization, FeatureModule) on the CPU.

    CPC_REFERENCE=/path/to/reference PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_features.py [--check]

The reference is imported unmodified.  torchaudio is a stub whose load() serves tensors by key, progressbar is an empty stub,
Tensor.cuda / Module.cuda are the identity.  Only data is written: inputs, outputs, case lists.  --check regenerates everything
and compares with the committed files (values to 1e-6) instead of writing.

Two parts:
  a. provenance sweep -- the readers run on tests/features_probe.py's ProbeMaker and the waveform arange(n); the output (which
     sample every frame starts at, the length and the row count of the call it came from) is stored run-length coded
     (features_probe.encode, lossless) as int64, or the fact that the reference raised.  A few cases with seqNorm as floats.
  b. values -- the reference's models in float64 (stored rounded to f32), the f32 run's distance to it in the json.  Models:
     tests/golden/ref_checkpoint (hidden 32, written by the reference) and oracle/synth parameters in the reference's classes at
     hidden 256 / 512.  The wide models' outputs are stored on 64 fixed channels (chan/<model>) to keep the files small; the
     json has the full shape.  g25_features.npz: waveform, sweep, hidden 32; g25_features_wide.npz: hidden 256 / 512.
"""
import argparse
import copy
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
REF = os.environ.get("CPC_REFERENCE")
if not REF or not os.path.isdir(os.path.join(REF, "cpc")):
    sys.exit("CPC_REFERENCE must name a checkout of the reference (the directory that holds cpc/)")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WAVES = {}
_ta = types.ModuleType("torchaudio")
_ta.load = lambda key: (WAVES[key], 16000)
sys.modules["torchaudio"] = _ta
sys.modules.setdefault("progressbar", types.ModuleType("progressbar"))
torch.Tensor.cuda = lambda self, *a, **k: self
torch.nn.Module.cuda = lambda self, *a, **k: self
sys.path.insert(0, REF)
import cpc.feature_loader as ref_fl        # noqa: E402
import cpc.model as ref_model              # noqa: E402
import cpc.transformers as ref_tr          # noqa: E402

import features_probe as FP                # noqa: E402

torch.set_num_threads(1)
N_WAVE = 36900
SHORT_RESTS = (159, 160, 319, 320, 399)
WIDE = {       # oracle/synth parameters in the reference's classes
    "gru256": dict(hidden=256, ar="GRU", layers=1, enc_seed=31, ar_seed=32),
    "lstm256x2": dict(hidden=256, ar="LSTM", layers=2, enc_seed=31, ar_seed=33),
    "gru512x2": dict(hidden=512, ar="GRU", layers=2, enc_seed=34, ar_seed=35),
    "tr256": dict(hidden=256, ar="transformer", layers=1, size_seq=128, enc_seed=31, ar_seed=36),
}


def waveform():
    rs = np.random.RandomState(2500)
    t = np.arange(N_WAVE) / 16000.0
    return (0.1 * np.sin(2 * np.pi * 220.0 * t) + 0.03 * rs.standard_normal(N_WAVE)).astype(np.float32)


def call(reader, maker, key, strict, C, seqNorm, bs):
    with torch.no_grad():
        if reader == "buildFeature":
            return ref_fl.buildFeature(maker, key, strict=strict, maxSizeSeq=C, seqNorm=seqNorm)
        return ref_fl.buildFeature_batch(maker, key, strict=strict, maxSizeSeq=C, seqNorm=seqNorm, batch_size=bs)


# --------------------------------------------------------------------------- a. provenance
def provenance(arr, meta):
    probe = FP.ProbeMaker()
    raised = {}
    for case in FP.sweep_cases():
        reader, C, strict, bs, n = case
        WAVES["probe"] = torch.arange(n, dtype=torch.float32).view(1, -1)
        key = FP.sweep_key(case)
        try:
            arr[key] = FP.encode(call(reader, probe, "probe", strict, C, False, bs))
        except Exception as e:                                   # the FACT that the reference raised is the record
            raised[key] = type(e).__name__
    norm = []
    for reader, C, bs in (("buildFeature", 8000, 0), ("buildFeature", 10000, 0), ("buildFeature_batch", 8000, 3),
                          ("buildFeature_batch", 10000, 3)):
        for strict in (False, True):
            n = 3 * C + 6900
            WAVES["probe"] = torch.arange(n, dtype=torch.float32).view(1, -1)
            key = f"provnorm/{reader}/C{C}/{'strict' if strict else 'loose'}/b{bs}/n{n}"
            arr[key] = call(reader, probe, "probe", strict, C, True, bs)[0].numpy()
            norm.append(dict(key=key, reader=reader, maxSizeSeq=C, strict=strict, batch_size=bs, n=n))
    meta["provenance"] = dict(cases=len(FP.sweep_cases()), raised=raised, seqnorm=norm)


# --------------------------------------------------------------------------- b. values
def checkpoint_model():
    run = os.path.join(OUT, "ref_checkpoint")
    with open(os.path.join(run, "checkpoint_args.json")) as f:
        args = argparse.Namespace(**json.load(f))
    model = ref_model.CPCModel(ref_fl.getEncoder(args), ref_fl.getAR(args))
    model.load_state_dict(torch.load(os.path.join(run, "checkpoint_7.pt"), "cpu")["gEncoder"], strict=False)
    return model.eval()


def wide_model(cfg):
    h = cfg["hidden"]
    enc = ref_model.CPCEncoder(h, "layerNorm")
    if cfg["ar"] == "transformer":
        ar = ref_tr.buildTransformerAR(h, h, cfg["layers"], cfg["size_seq"], False)
    else:
        ar = ref_model.CPCAR(h, h, False, cfg["layers"], mode=cfg["ar"])
    model = ref_model.CPCModel(enc, ar)
    sd = FP.wide_params(cfg)
    sd.update({k: v for k, v in model.state_dict().items() if k.endswith(".z") or k.endswith(".mask")})
    model.load_state_dict(sd)
    return model.eval()


class Recorder:
    """Runs one case on the f64 and the f32 copy of a model and files the results."""

    def __init__(self, name, model, wave, arr, cases, channels=None):
        self.name, self.arr, self.cases = name, arr, cases
        self.m32, self.m64 = model, copy.deepcopy(model).double()
        self.w32 = torch.from_numpy(wave).view(1, -1)
        self.w64 = self.w32.double()
        self.ch = channels

    def pick(self, x):
        """[1, frames, dim] -> f32 [frames, stored channels]"""
        x = x[0] if self.ch is None else x[0][:, self.ch]
        return x.float().numpy()

    def run(self, model, wave, reader, enc, strict, C, seqNorm, bs, start, n):
        WAVES["w"] = wave[:, start:start + n]
        return call(reader, ref_fl.FeatureModule(model, enc).eval(), "w", strict, C, seqNorm, bs)

    def spans(self, reader, strict, C, n):
        """[(frames of the call, frames kept)] per span, read off the probe (the reference's own plan, not a restatement)."""
        WAVES["probe"] = torch.arange(n, dtype=torch.float32).view(1, -1)
        out = []
        for first, count, length, rows in FP.encode(call(reader, FP.ProbeMaker(), "probe", strict, C, False, bs=3)):
            per, count = FP.frames(int(length)), int(count)
            out += [(per, per)] * (count // per)
            if count % per:
                out.append((per, count % per))            # a strict tail: the last frames of a whole chunk
        return out

    def case(self, tag, reader, enc, strict, C, seqNorm, bs, start, n):
        cid = f"{self.name}/{tag}"
        ref = self.run(self.m64, self.w64, reader, enc, strict, C, seqNorm, bs, start, n)
        f32 = self.run(self.m32, self.w32, reader, enc, strict, C, seqNorm, bs, start, n)
        spans = self.spans(reader, strict, C, n)
        assert sum(k for _, k in spans) == ref.shape[1], (cid, spans, ref.shape)
        rec = dict(id=cid, model=self.name, reader=reader, get_encoded=enc, strict=strict, maxSizeSeq=C, seqNorm=seqNorm,
                   batch_size=bs, start=start, n=n, shape=list(ref.shape), spans=[list(s) for s in spans],
                   ref_max=float(ref.abs().max()), f32_dist=float((f32.double() - ref).abs().max()))
        self.arr[f"val/{cid}"] = self.pick(ref)
        if seqNorm:
            # per span and channel: sqrt(var + 1e-8) of the raw f64 span, and (strict) the whole raw tail span
            raw = self.run(self.m64, self.w64, reader, enc, False, C, False, bs, start, n)
            raw32 = self.run(self.m32, self.w32, reader, enc, strict, C, False, bs, start, n)
            rawref = self.run(self.m64, self.w64, reader, enc, strict, C, False, bs, start, n)
            rec["raw_max"] = float(rawref.abs().max())
            rec["f32_raw_dist"] = float((raw32.double() - rawref).abs().max())
            pieces, at = [], 0
            for i, (per, kept) in enumerate(spans):
                if kept == per:
                    pieces.append(raw[:, at:at + per])
                    at += per
                else:
                    WAVES["w"] = self.w64[:, start + n - C:start + n]
                    with torch.no_grad():
                        tail = ref_fl.FeatureModule(self.m64, enc).eval()((WAVES["w"].view(1, 1, -1), None))
                    assert tail.shape[1] == per
                    pieces.append(tail)
                    self.arr[f"rawtail/{cid}"] = self.pick(tail)
            std = torch.stack([torch.sqrt(p.var(dim=1)[0] + 1e-8) for p in pieces])             # [spans, dim], f64
            self.arr[f"std/{cid}"] = std.numpy() if self.ch is None else std[:, self.ch].numpy()
        self.cases.append(rec)
        return rec

    def keep_hidden(self, C, files):
        """One feature maker with keepHidden, called on file A, then B, then A again: the state is never reset."""
        out = {}
        for model, wave, kind in ((self.m64, self.w64, "f64"), (self.m32, self.w32, "f32")):
            model.gAR.keepHidden = True
            model.gAR.hidden = None
            maker = ref_fl.FeatureModule(model, False).eval()
            res = []
            for start, n in files:
                WAVES["w"] = wave[:, start:start + n]
                with torch.no_grad():
                    res.append(ref_fl.buildFeature(maker, "w", strict=False, maxSizeSeq=C, seqNorm=False))
            model.gAR.keepHidden = False
            model.gAR.hidden = None
            out[kind] = res
        recs = []
        for i, ((start, n), ref, f32) in enumerate(zip(files, out["f64"], out["f32"])):
            cid = f"{self.name}/keepHidden/{i}"
            self.arr[f"val/{cid}"] = self.pick(ref)
            recs.append(dict(id=cid, start=start, n=n, shape=list(ref.shape), ref_max=float(ref.abs().max()),
                             f32_dist=float((f32.double() - ref).abs().max())))
        first_again = float((out["f64"][2] - out["f64"][0]).abs().max())
        return dict(model=self.name, maxSizeSeq=C, calls=recs, third_call_differs_from_first_by=first_again)


def values(arr32, arrw, meta):
    wave = waveform()
    arr32["wave"] = wave
    cases, keep = [], []
    # hidden 32, the checkpoint the reference wrote: the full matrix on the whole waveform ...
    r = Recorder("h32", checkpoint_model(), wave, arr32, cases)
    for reader, C, bs in (("buildFeature", 10000, 0), ("buildFeature_batch", 8000, 3)):
        short = "bf" if reader == "buildFeature" else "bb"
        for enc in (False, True):
            for strict in (False, True):
                for seqNorm in (False, True):
                    tag = f"{short}/{'enc' if enc else 'ctx'}/{'strict' if strict else 'loose'}/{'norm' if seqNorm else 'raw'}/full"
                    rec = r.case(tag, reader, enc, strict, C, seqNorm, bs, 0, N_WAVE)
                    if seqNorm:
                        rec["raw_of"] = f"h32/{tag.replace('/norm/', '/raw/')}"
        # ... and one chunk plus a rest of 1 or 2 frames, the lengths the non-strict rest feeds on its own
        for rest in SHORT_RESTS:
            for enc, strict in ((False, False), (True, False), (False, True)):
                tag = f"{short}/{'enc' if enc else 'ctx'}/{'strict' if strict else 'loose'}/raw/rest{rest}"
                r.case(tag, reader, enc, strict, C, False, bs, 0, C + rest)
    keep.append(r.keep_hidden(10000, [(0, 12500), (14000, 11700), (0, 12500)]))
    # hidden 256 / 512: three chunks of 4000 and a rest, 64 channels stored
    n_wide = 3 * 4000 + 1900
    enc_done = set()
    for name, cfg in WIDE.items():
        ch = np.sort(np.random.RandomState(25).choice(cfg["hidden"], 64, replace=False))
        arrw[f"chan/{name}"] = ch.astype(np.int64)
        r = Recorder(name, wide_model(cfg), wave, arrw, cases, channels=torch.from_numpy(ch))
        if (cfg["hidden"], cfg["enc_seed"]) not in enc_done:          # (the 256-wide models share one encoder)
            enc_done.add((cfg["hidden"], cfg["enc_seed"]))
            r.case("bf/enc/loose/raw/full", "buildFeature", True, False, 4000, False, 0, 0, n_wide)
            r.case("bf/enc/strict/norm/full", "buildFeature", True, True, 4000, True, 0, 0, n_wide)
            r.case("bf/enc/loose/raw/rest319", "buildFeature", True, False, 4000, False, 0, 0, 4000 + 319)
            r.case("bb/enc/loose/raw/rest160", "buildFeature_batch", True, False, 4000, False, 3, 0, 8000 + 160)
        r.case("bf/ctx/loose/norm/full", "buildFeature", False, False, 4000, True, 0, 0, n_wide)
        r.case("bb/ctx/strict/raw/full", "buildFeature_batch", False, True, 4000, False, 3, 0, n_wide)
        r.case("bf/ctx/loose/raw/rest160", "buildFeature", False, False, 4000, False, 0, 0, 4000 + 160)
        r.case("bb/ctx/loose/raw/rest399", "buildFeature_batch", False, False, 4000, False, 3, 0, 8000 + 399)
        if cfg["ar"] != "transformer":
            keep.append(r.keep_hidden(10000, [(0, 12500), (14000, 11700), (0, 12500)]))
    meta["models"] = WIDE
    meta["cases"] = cases
    meta["keepHidden"] = keep


def compare(name, new):
    old = np.load(os.path.join(OUT, name), allow_pickle=False)
    assert sorted(old.files) == sorted(new), f"{name}: the keys differ"
    worst = 0.0
    for k, v in new.items():
        v = np.asarray(v)
        assert old[k].shape == v.shape and old[k].dtype == v.dtype, k
        if v.size:
            worst = max(worst, float(np.abs(old[k].astype(np.float64) - v.astype(np.float64)).max()))
    assert worst <= 1e-6, f"{name}: differs from the committed file by {worst:.2e}"
    print(f"{name}: reproduced, max difference {worst:.1e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    opt = ap.parse_args()
    arr32, arrw, meta = {}, {}, {"torch_version": torch.__version__}
    provenance(arr32, meta)
    values(arr32, arrw, meta)
    if opt.check:
        compare("g25_features.npz", arr32)
        compare("g25_features_wide.npz", arrw)
        return
    for name, arr in (("g25_features.npz", arr32), ("g25_features_wide.npz", arrw)):
        np.savez_compressed(os.path.join(OUT, name), **arr)
        print("wrote", name, os.path.getsize(os.path.join(OUT, name)), "bytes")
    with open(os.path.join(OUT, "g25_features.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote g25_features.json", os.path.getsize(os.path.join(OUT, "g25_features.json")), "bytes")


if __name__ == "__main__":
    main()
