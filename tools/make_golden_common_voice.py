#!/usr/bin/env python3
"""Generate tests/golden/g27_common_voice.npz and tests/golden/g27_phone_transcripts.txt: the REFERENCE's
cpc/eval/common_voices_eval.py run on the CPU, and the transcriptions the whole-utterance tests read.

Needs a checkout of the reference repository (the directory that holds its `cpc` package) and the built library (the audio
files are decoded by cpc2_amd.audio); run from the repository root:
    CPC_REFERENCE=DIR PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_common_voice.py

The reference's file is imported unmodified; torchaudio, augment, torch_audiomentations, progressbar and psutil are registered as
stand-in modules, as tools/make_golden_augment.py does.  `torchaudio.load` serves what cpc2_amd.audio.load returns for the same
file, and the module's `Pool` name is rebound to a stand-in that maps in this process.  CTCphone_criterion.forward is NOT
recorded: it does not run on a current torch (integer `/=`), see cpc2_amd/eval/common_voices_eval.py.  Only data is written.

g27_phone_transcripts.txt: one line `name l0 l1 ...` for each of the nine utterances of tests/golden/test_db -- the collapsed
frame labels of tests/golden/phone_labels.txt where it has the utterance, else frames // 12 labels drawn from
numpy.random.default_rng(27) (a transcription need not be true to test the arithmetic); 41 phones.

g27_common_voice.npz:
  * `sd_keys`, `sd_{key}_shape`, `sd_{key}_abssum`: the state dict of CTCphone_criterion(32, 5) after torch.manual_seed(27).
  * `gp{i}_*`: getPrediction in float64 (torch's default dtype set to float64 for the call: the seqNorm branch allocates its
    buffer in the default dtype) for {seqNorm} x {LSTM} at H = 32, nPhones = 5, B = 3, S = 40, sizes (40, 33, 21): the input `c`,
    every parameter `p_{key}`, the output `pred`.
  * `ds_*`: SingleSequenceDataset over the nine utterances: names in load order, seqOffset, phoneOffsets, maxSize, maxSizePhone,
    and for random_offset_amplitude 0 (`ds0_*`) and 80 after random.seed(27) (`ds80_*`, items 0 .. 8 in order) per item the two
    sizes, the phone row, the float64 sum of the audio row, its first 8 samples and the 8 around its end.
  * `cut_*`: cut_data on a [4, 10, 3] array.
  * `per{i}_*`: get_per on recorded probabilities (tie-free by tests/per_oracle.py, as tools/make_golden_per.py enforces).
"""
import importlib.util
import json
import os
import random
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("CPC_REFERENCE")
if not REF or not os.path.isdir(os.path.join(REF, "cpc")):
    raise SystemExit("set CPC_REFERENCE to a checkout of the reference repository (the directory that holds cpc/)")
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import per_oracle  # noqa: E402
from cpc2_amd import audio as our_audio  # noqa: E402
from cpc2_amd.dataset import findAllSeqs, parseSeqLabels  # noqa: E402

for name in ("torchaudio", "augment", "augment.effects", "torch_audiomentations", "progressbar", "psutil"):
    sys.modules[name] = types.ModuleType(name)
sys.modules["augment"].effects = sys.modules["augment.effects"]
sys.modules["augment.effects"].EffectChain = object
for name in ("Compose", "AddBackgroundNoise", "ApplyImpulseResponse"):
    setattr(sys.modules["torch_audiomentations"], name, None)
sys.modules["torchaudio"].load = lambda path: our_audio.load(path)
sys.path.insert(0, REF)
_spec = importlib.util.spec_from_file_location("ref_common_voices_eval", os.path.join(REF, "cpc", "eval", "common_voices_eval.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)


class _SerialPool:
    def __init__(self, _n):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def map(self, fn, items):
        return [fn(x) for x in items]


ref.Pool = _SerialPool
ARR = {}
META = {}


def transcripts():
    frame_labels, _ = parseSeqLabels(os.path.join(GOLDEN, "phone_labels.txt"))
    seqs, _ = findAllSeqs(os.path.join(GOLDEN, "test_db"), extension=".flac")
    rng = np.random.default_rng(27)
    lines = []
    for _, rel in sorted(seqs, key=lambda x: os.path.basename(x[1])):
        name = os.path.splitext(os.path.basename(rel))[0]
        if name in frame_labels:
            lab = np.asarray(frame_labels[name])
            lab = lab[np.concatenate([[True], lab[1:] != lab[:-1]])]
        else:
            frames = our_audio.info(os.path.join(GOLDEN, "test_db", rel))[2] // 160
            lab = rng.integers(0, 41, frames // 12)
        lines.append(name + " " + " ".join(str(int(v)) for v in lab))
    path = os.path.join(GOLDEN, "g27_phone_transcripts.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path, seqs


def state_dict():
    torch.manual_seed(27)
    crit = ref.CTCphone_criterion(32, 5)
    keys = list(crit.state_dict().keys())
    ARR["sd_keys"] = np.array(json.dumps(keys))
    for k, v in crit.state_dict().items():
        ARR[f"sd_{k}_shape"] = np.array(v.shape, np.int64)
        ARR[f"sd_{k}_abssum"] = np.float64(v.double().abs().sum().item())


def predictions():
    torch.set_default_dtype(torch.float64)
    try:
        i = 0
        for seq_norm in (False, True):
            for lstm in (False, True):
                torch.manual_seed(270 + i)
                crit = ref.CTCphone_criterion(32, 5, LSTM=lstm, seqNorm=seq_norm).double().eval()
                c = torch.randn(3, 40, 32) * (1.0 + torch.arange(32) / 16.0) + torch.linspace(-1, 1, 32)
                sizes = torch.tensor([40, 33, 21])
                with torch.no_grad():
                    pred = crit.getPrediction(c, sizes)
                assert pred.shape == (3, 9, 6) and pred.dtype == torch.float64
                ARR[f"gp{i}_c"], ARR[f"gp{i}_sizes"], ARR[f"gp{i}_pred"] = c.numpy(), sizes.numpy(), pred.numpy()
                ARR[f"gp{i}_flags"] = np.array([int(seq_norm), int(lstm)])
                for k, v in crit.state_dict().items():
                    ARR[f"gp{i}_p_{k}"] = v.numpy()
                i += 1
    finally:
        torch.set_default_dtype(torch.float32)


def dataset(path_transcripts, seqs):
    labels, n_phones = parseSeqLabels(path_transcripts)
    assert n_phones == 41
    db = os.path.join(GOLDEN, "test_db")
    for amp in (0, 80):
        ds = ref.SingleSequenceDataset(db, seqs, labels, random_offset_amplitude=amp)
        if amp == 0:
            ARR["ds_names"] = np.array(json.dumps(sorted(os.path.splitext(os.path.basename(r))[0] for _, r in seqs)))
            ARR["ds_seqOffset"] = np.array(ds.seqOffset, np.int64)
            ARR["ds_phoneOffsets"] = np.array(ds.phoneOffsets, np.int64)
            ARR["ds_maxSize"], ARR["ds_maxSizePhone"], ARR["ds_len"] = np.int64(ds.maxSize), np.int64(ds.maxSizePhone), np.int64(len(ds))
        random.seed(27)
        rows = dict(sizeSeq=[], sizePhone=[], phone=[], sum=[], head=[], edge=[])
        for idx in range(len(ds)):
            seq, size_seq, phone, size_phone = ds[idx]
            assert seq.shape == (1, ds.maxSize) and phone.dtype == torch.long
            n = int(size_seq)
            rows["sizeSeq"].append(n)
            rows["sizePhone"].append(int(size_phone))
            rows["phone"].append(phone.numpy())
            rows["sum"].append(seq.double().sum().item())
            rows["head"].append(seq[0, :8].numpy())
            edge = torch.zeros(8)
            got = seq[0, n - 4:n + 4]
            edge[:got.numel()] = got
            rows["edge"].append(edge.numpy())
        for k, v in rows.items():
            ARR[f"ds{amp}_{k}"] = np.array(v)


def cut():
    g = torch.Generator().manual_seed(27)
    seq = torch.randn(4, 10, 3, generator=g)
    sizes = torch.tensor([3, 7, 5, 1])
    ARR["cut_in"], ARR["cut_sizes"], ARR["cut_out"] = seq.numpy(), sizes.numpy(), ref.cut_data(seq, sizes).numpy()


def pers():
    cases = [(30, 6, 100, 9), (24, 42, 97, 14), (12, 6, 200, 5)]
    for i, (t, p, size_pred, size_gt) in enumerate(cases):
        for seed in range(32):
            g = torch.Generator().manual_seed(2700 + 32 * i + seed)
            path = torch.randint(0, p, (t,), generator=g)
            logits = torch.randn(t, p, generator=g)
            logits[torch.arange(t), path] += 3.0
            pred = torch.softmax(logits, 1)
            gt = torch.randint(0, p - 1, (size_gt + 3,), generator=g)
            l_ = min(size_pred // 4, t)
            if not per_oracle.beam_search(pred[:l_].numpy(), 20, p - 1)[1]:
                break
        else:
            raise SystemExit(f"get_per case {i}: no tie-free seed in 0 .. 31")
        value = ref.get_per((pred, size_pred, gt, size_gt, p - 1))
        ARR[f"per{i}_pred"], ARR[f"per{i}_gt"] = pred.numpy(), gt.numpy()
        ARR[f"per{i}_args"] = np.array([size_pred, size_gt, p - 1], np.int64)
        ARR[f"per{i}_value"] = np.float64(value)
        print(f"get_per case {i}: seed {seed} PER {value}")
    META["n_per"] = len(cases)


def main():
    path_transcripts, seqs = transcripts()
    state_dict()
    predictions()
    dataset(path_transcripts, seqs)
    cut()
    pers()
    ARR["meta"] = np.array(json.dumps(META))
    path = os.path.join(GOLDEN, "g27_common_voice.npz")
    np.savez_compressed(path, **ARR)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
