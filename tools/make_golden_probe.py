#!/usr/bin/env python3
"""Generate tests/golden/g21_linear_separability.npz (and copy the reference's phone label fixture to
tests/golden/phone_labels.txt) by running the REFERENCE's linear-separability pieces on the CPU.

Needs a checkout of the reference repository (the directory that holds its `cpc` package):
    CPC_REFERENCE=DIR PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_probe.py

The reference is imported unmodified.  progressbar is stubbed, and so is torchaudio, whose load / info are served by
cpc2_amd.audio so that the reference's own AudioBatchData reads the committed FLACs.  Recorded:
  * parseSeqLabels of the fixture (nPhones, and the label lists of the two labelled files of tests/golden/test_db);
  * AudioBatchData.getPhonem of window offsets over those two files (offsets that are not multiples of 160, windows that
    straddle the file boundary) and collapseLabelChain of batches of them;
  * PhoneCriterion (1 and 2 layers), SpeakerCriterion and CTCPhoneCriterion from seeded inits, on the context features of
    tests/golden/ref_checkpoint/checkpoint_7.pt over two labelled windows: loss, accuracy, the gradients of every weight and
    bias, the feature gradient projected on 8 fixed directions, the same in float64 for CTC, and 20 steps of
    torch.optim.Adam(lr=2e-4, eps=2e-8) on fixed batches (loss trajectory, final parameters).
"""
import json
import os
import shutil
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("CPC_REFERENCE")
if not REF or not os.path.isdir(os.path.join(REF, "cpc")):
    raise SystemExit("set CPC_REFERENCE to a checkout of the reference repository (the directory that holds cpc/)")
OUT = os.path.join(ROOT, "tests", "golden")
DB = os.path.join(OUT, "test_db")
CKPT = os.path.join(OUT, "ref_checkpoint", "checkpoint_7.pt")
sys.path.insert(0, ROOT)
from cpc2_amd import audio  # noqa: E402


class _ProgressBar:
    def __init__(self, *a, **k):
        pass

    def start(self):
        pass

    def update(self, *a):
        pass

    def finish(self):
        pass


sys.modules["progressbar"] = types.SimpleNamespace(ProgressBar=_ProgressBar)
_ta = types.ModuleType("torchaudio")
_ta.load = lambda path, *a, **k: audio.load(path)
_ta.info = lambda path, *a, **k: types.SimpleNamespace(num_frames=audio.info(path)[2])
sys.modules["torchaudio"] = _ta
sys.path.insert(0, REF)
import cpc.criterion as ref_cr  # noqa: E402
from cpc.criterion.seq_alignment import collapseLabelChain  # noqa: E402
from cpc.dataset import AudioBatchData, findAllSeqs, parseSeqLabels  # noqa: E402
import cpc.feature_loader as ref_fl  # noqa: E402

ARR = {}
META = {}
LABELLED = ["2911-12359-0007", "4051-11218-0044"]
N_STEPS = 20


def labels_and_windows():
    labels, n_phones = parseSeqLabels(os.path.join(REF, "cpc", "test_data", "phone_labels.txt"))
    META["n_phones"] = n_phones
    META["n_label_lines"] = len(labels) - 1
    META["step"] = labels["step"]
    for name in LABELLED:
        ARR[f"labels_{name}"] = np.array(labels[name], np.int64)
    cache = os.path.join(tempfile.mkdtemp(prefix="g21_"), "seqs_cache.txt")     # (not under the committed data)
    seqs, speakers = findAllSeqs(DB, extension=".flac", cache_path=cache)
    META["n_speakers"] = len(speakers)
    chosen = sorted([s for s in seqs if os.path.splitext(os.path.basename(s[1]))[0] in LABELLED])
    META["seqs"] = [list(s) for s in chosen]
    db = AudioBatchData(DB, 20480, chosen, labels, len(speakers), nProcessLoader=1)
    n = len(db.data)
    boundary = db.seqLabel[1]
    META["data_size"] = n
    META["seq_label"] = list(db.seqLabel)
    META["speaker_label"] = list(db.speakerLabel)
    offsets = [0, 1, 159, 160, 161, 5000, 12345, 20480, 30001, boundary - 20480, boundary - 20479, boundary - 10000,
               boundary - 161, boundary - 1, boundary, boundary + 79, n - 20480 - 1, n - 20480]
    offsets = [o for o in offsets if 0 <= o <= n - 20480]
    ARR["offsets"] = np.array(offsets, np.int64)
    ARR["phonem"] = np.stack([np.array(db.getPhonem(o), np.int64) for o in offsets])
    ARR["speaker_of_offset"] = np.array([db.getSpeakerLabel(o) for o in offsets], np.int64)
    for tag, rows in (("all", slice(None)), ("three", slice(2, 5)), ("one", slice(7, 8))):
        out, sizes = collapseLabelChain(torch.from_numpy(ARR["phonem"][rows]))
        ARR[f"collapse_{tag}_out"] = out.numpy()
        ARR[f"collapse_{tag}_sizes"] = sizes.numpy()
    return db, labels, n_phones, len(speakers)


def features(db):
    # (the checkpoint's args predate the `load` entry reference loadModel reads: the model is built as it builds it, from the
    #  default configuration overlaid with the run's args)
    from cpc.cpc_default_config import get_default_cpc_config
    from cpc.model import CPCModel
    _, _, run_args = ref_fl.getCheckpointData(os.path.dirname(CKPT))
    args = get_default_cpc_config()
    ref_fl.loadArgs(args, run_args)
    model = CPCModel(ref_fl.getEncoder(args), ref_fl.getAR(args))
    model.load_state_dict(torch.load(CKPT, "cpu")["gEncoder"], strict=False)
    hidden_gar, hidden_encoder = args.hiddenGar, args.hiddenEncoder
    model.eval()
    win = [12345, db.seqLabel[1] - 10000]             # the second window straddles the file boundary
    x = torch.stack([db.data[o:o + 20480] for o in win]).view(len(win), 1, 20480)
    with torch.no_grad():
        c, enc, _ = model(x, None)
    ARR["feat_offsets"] = np.array(win, np.int64)
    ARR["cfeature"] = c.numpy().astype(np.float32)
    META["hidden_gar"], META["hidden_encoder"] = hidden_gar, hidden_encoder
    phon = torch.tensor(np.stack([np.array(db.getPhonem(o), np.int64) for o in win]))
    spk = torch.tensor([db.getSpeakerLabel(o) for o in win], dtype=torch.long)
    return c.contiguous(), phon, spk


def criterion_case(tag, make, seed, c, label):
    torch.manual_seed(seed)
    crit = make()
    proj = torch.from_numpy(np.random.default_rng(21).standard_normal((c.shape[2], 8)))
    feat = c.clone().requires_grad_(True)
    loss, acc = crit(feat, feat, label)
    loss.sum().backward()
    ARR[f"{tag}_loss"] = loss.detach().numpy().astype(np.float64)
    ARR[f"{tag}_acc"] = acc.detach().numpy().astype(np.float64)
    for name, p in crit.named_parameters():
        ARR[f"{tag}_grad_{name}"] = p.grad.numpy()
    ARR[f"{tag}_dX_proj"] = (feat.grad.double() @ proj).numpy()
    META[tag] = dict(seed=seed, keys=list(crit.state_dict().keys()))
    if tag == "ctc":
        # the same criterion in float64: torch's f32 CTC runs its alpha / beta in f32 log space, whose rounding (one ulp of
        # |log alpha| ~ 100-500) reaches the gradient at ~1e-5 -- the f64 run is the reference's semantics without it
        torch.manual_seed(seed)
        crit64 = make().double()
        feat64 = c.double().clone().requires_grad_(True)
        loss64, _ = crit64(feat64, feat64, label)
        loss64.sum().backward()
        ARR["ctc64_loss"] = loss64.detach().numpy()
        for name, p in crit64.named_parameters():
            ARR[f"ctc64_grad_{name}"] = p.grad.numpy()
        ARR["ctc64_dX_proj"] = (feat64.grad @ proj).numpy()
    # 20 Adam steps on fixed batches: window 0, window 1, both, repeated
    torch.manual_seed(seed)
    crit = make()
    opt = torch.optim.Adam(crit.parameters(), lr=2e-4, eps=2e-8)
    batches = [slice(0, 1), slice(1, 2), slice(0, 2)]
    traj = []
    for i in range(N_STEPS):
        rows = batches[i % 3]
        opt.zero_grad()
        loss, _ = crit(c[rows], c[rows], label[rows])
        loss.sum().backward()
        opt.step()
        traj.append(float(loss.item()))
    ARR[f"{tag}_traj"] = np.array(traj)
    for name, p in crit.named_parameters():
        ARR[f"{tag}_final_{name}"] = p.detach().numpy()


def parse_defaults():
    import cpc.eval.linear_separability as ref_ls
    a = vars(ref_ls.parse_args(["db", "train.txt", "val.txt", "ckpt.pt"]))
    a["load"] = ["ckpt.pt"]
    a["pathCheckpoint"] = "out"
    a.pop("nGPU")                                      # (torch.cuda.device_count() of the machine that ran it)
    META["parse_args_defaults"] = a


def main():
    db, labels, n_phones, n_speakers = labels_and_windows()
    c, phon, spk = features(db)
    H = c.shape[2]
    criterion_case("phone1", lambda: ref_cr.PhoneCriterion(H, n_phones, False), 1, c, phon)
    criterion_case("phone2", lambda: ref_cr.PhoneCriterion(H, n_phones, False, nLayers=2), 2, c, phon)
    criterion_case("speaker", lambda: ref_cr.SpeakerCriterion(H, n_speakers), 3, c, spk)
    criterion_case("ctc", lambda: ref_cr.CTCPhoneCriterion(H, n_phones, False), 4, c, phon)
    parse_defaults()
    ARR["meta"] = np.array(json.dumps(META, default=str))
    path = os.path.join(OUT, "g21_linear_separability.npz")
    np.savez_compressed(path, **ARR)
    shutil.copyfile(os.path.join(REF, "cpc", "test_data", "phone_labels.txt"), os.path.join(OUT, "phone_labels.txt"))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
