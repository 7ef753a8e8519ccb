#!/usr/bin/env python3
"""Generate tests/golden/g23_train_cli.json by running the REFERENCE's command line pieces on the CPU.

Needs a checkout of the reference repository (the directory that holds its `cpc` package); run from the repository root:
    CPC_REFERENCE=DIR PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_train_cli.py

The reference is imported unmodified; torchaudio, augment, torch_audiomentations, progressbar and psutil are registered as
empty modules (nothing recorded here decodes audio).  Recorded, as data only:
  * `parse`: cpc.train.parseArgs for a list of command lines.  Paths under the repository root are written as $ROOT/...;
    every command line gives --nGPU 0 and --random_seed so that nothing depends on the box;
  * `find`: cpc.dataset.findAllSeqs over trees of EMPTY files (the names are in the JSON), one tree per naming convention,
    with and without no_speaker -- each sequence with its speaker NAME (the index follows os.walk order, which differs
    from box to box).  No two files of a tree share a sort key: ties keep os.walk order;
  * `artefacts`: AudioLoader.__remove_artefacts on a stand-in data set (seqLabel, sizeWindow) for batches of
    SameSpeakerSampler and TemporalSameSpeakerSampler and for hand-made batches that hit every branch;
  * `split`: the (train, validation) lists cpc.train.main hands to AudioBatchData for tests/golden/test_db, AudioBatchData
    being replaced by a recorder that raises on its second call: with --pathTrain (the list is then sorted by name before the
    shuffle) and with temporalsamespeaker + spkr-id, two seeds each.  test_db holds files that tie under spkr-id (same speaker
    and chapter) and keep os.walk order: the seeds of that case are the first two for which the validation file (the last of
    the shuffled list) is a speaker's only file, so that the lists do not depend on the box beyond the order inside a tie.
"""
import contextlib
import io
import json
import os
import random
import sys
import tempfile
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("CPC_REFERENCE")
if not REF or not os.path.isdir(os.path.join(REF, "cpc")):
    raise SystemExit("set CPC_REFERENCE to a checkout of the reference repository (the directory that holds cpc/)")
OUT = os.path.join(ROOT, "tests", "golden", "g23_train_cli.json")
DB = os.path.join(ROOT, "tests", "golden", "test_db")
for name in ("torchaudio", "augment", "augment.effects", "torch_audiomentations", "progressbar", "psutil"):
    sys.modules[name] = types.ModuleType(name)
sys.modules["augment"].effects = sys.modules["augment.effects"]
for name in ("Compose", "AddBackgroundNoise", "ApplyImpulseResponse"):          # (imported by name, never called here)
    setattr(sys.modules["torch_audiomentations"], name, None)
sys.path.insert(0, REF)
os.chdir(ROOT)
import cpc.dataset as ref_ds  # noqa: E402
import cpc.train as ref_train  # noqa: E402


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def rootless(value):
    if isinstance(value, str) and value.startswith(ROOT):
        return "$ROOT" + value[len(ROOT):]
    if isinstance(value, list):
        return [rootless(v) for v in value]
    return value


# ----------------------------------------------------------------------------- parseArgs
BOX = ["--nGPU", "0", "--random_seed", "11"]
COMMAND_LINES = {
    "defaults": ["--pathDB", "db"] + BOX,
    "recipe": ["--pathDB", "db", "--pathCheckpoint", "out/run", "--nLevelsGRU", "2", "--multihead_rnn", "--schedulerRamp", "10",
               "--save_step", "5", "--no_artefacts", "--samplingType", "samespeaker"] + BOX,
    "no_ar": ["--pathDB", "db", "--arMode", "no_ar", "--hiddenEncoder", "64", "--hiddenGar", "32"] + BOX,
    "relative_paths": ["--pathDB", "db", "--pathCheckpoint", "out/../out2", "--load", "a/checkpoint_3.pt", "--loadCriterion"] + BOX,
    "temporal": ["--pathDB", "db", "--samplingType", "temporalsamespeaker", "--naming_convention", "spkr-id", "--batchSizeGPU", "2",
                 "--optimizer", "sgd", "--ignore_cache", "--path_cache", "c.txt"] + BOX,
    "resume_only": ["--pathCheckpoint", "out/run", "--nEpoch", "5", "--learningRate", "0.001"] + BOX,
    "augment_flags": ["--pathDB", "db", "--augment_past", "--augment_type", "pitch", "additive", "--meta_aug", "--meta_aug_type",
                      "natural_reverb", "--pathDBNoise", "noise", "--t_ms", "50"] + BOX,
}


def record_parse():
    out = {}
    for tag, argv in COMMAND_LINES.items():
        args = quiet(ref_train.parseArgs, list(argv))
        out[tag] = {"argv": argv, "args": {k: rootless(v) for k, v in vars(args).items()}}
    return out


# ----------------------------------------------------------------------------- findAllSeqs
TREES = {
    "id_spkr_onset_offset": ["b/day2_anna_30.5_31.0.flac", "b/day2_anna_4.25_9.0.flac", "a/day1_bob_100.0_101.5.flac",
                             "a/day1_bob_20.0_21.0.flac", "a/day1_anna_7.0_8.0.flac", "a/day1_bob_3.5_4.0.flac", "a/skip.txt"],
    "id_spkr_onset_offset_spkr_onset_offset": ["x/day1_kid_12.0_13.0_mum_0.5_1.0.flac", "x/day1_kid_2.0_3.0_mum_5.0_6.0.flac",
                                               "x/day1_mum_7.5_8.0_kid_1.0_2.0.flac", "y/day3_kid_1.5_2.5_dad_9.0_9.5.flac",
                                               "y/day3_kid_0.5_1.0_dad_2.0_3.0.flac"],
    "spkr-id": ["103/1240/103-1240-0003.flac", "103/1240/notes.txt", "103/1241/103-1241-0000.flac", "27/90/27-90-0001.flac",
                "27/9/27-9-0005.flac", "27/100/27-100-0002.flac", "5/7/5-7-0000.flac"],
    "spkr_id_nb": ["s/anna_read_10.flac", "s/anna_read_9.flac", "s/anna_read_100.flac", "s/bob_talk_2.flac", "t/bob_talk_1.flac",
                   "t/carl_x_0.flac"],
    "spkr-id-nb": ["s/anna-read-10.flac", "s/anna-read-9.flac", "s/anna-read-100.flac", "s/bob-talk-2.flac", "t/bob-talk-1.flac",
                   "t/carl-x-0.flac"],
    "full_seedlings": ["h/01_06_12_v1.flac", "h/01_06_3_v1.flac", "h/01_06_7_v2.flac", "h/02_08_1_v1.flac", "g/02_08_0_v1.flac",
                       "g/03_09_5_v1.flac"],
    "no_speaker": ["p/rec_a_10.flac", "p/rec_a_9.flac", "p/rec_b_1.flac", "q/rec_a_11.flac", "q/tape_0.flac"],
}


def record_find():
    out = {}
    for convention, names in TREES.items():
        tmp = tempfile.mkdtemp(prefix="g23_tree_")
        for rel in names:
            os.makedirs(os.path.dirname(os.path.join(tmp, rel)), exist_ok=True)
            open(os.path.join(tmp, rel), "wb").close()
        cache = os.path.join(tempfile.mkdtemp(prefix="g23_cache_"), "cache.txt")
        entry = {"files": names}
        for no_speaker in (False, True):
            seqs, speakers = quiet(ref_ds.findAllSeqs, tmp, no_speaker=no_speaker, extension=".flac", format=convention,
                                   cache_path=cache)
            entry["no_speaker" if no_speaker else "speaker"] = {"speakers": sorted(speakers),
                                                                "seqs": [[speakers[i], rel] for i, rel in seqs]}
        out[convention] = entry
    return out


# ----------------------------------------------------------------------------- __remove_artefacts
class _StandIn:
    def __init__(self, seqLabel, sizeWindow):
        self.seqLabel, self.sizeWindow = seqLabel, sizeWindow


def _artefacts(seqLabel, sizeWindow, sampler):
    before = [list(b) for b in sampler.batches]
    loader = ref_ds.AudioLoader(_StandIn(seqLabel, sizeWindow), None, 1, None, 0, 0, remove_artefacts=True)
    after = quiet(loader._AudioLoader__remove_artefacts, sampler).batches
    return {"seqLabel": seqLabel, "sizeWindow": sizeWindow,
            "temporal": isinstance(sampler, ref_ds.TemporalSameSpeakerSampler), "before": before,
            "after": [list(b) for b in after]}


def record_artefacts():
    out = {}
    seqLabel = [0, 250, 600, 610, 1000, 1900, 2000]                # six sequences (one shorter than a window)
    speakerLabel = [0, 610, 1900, 2000]
    W = 100
    for offset in (0, 37):
        torch.manual_seed(5 + offset)
        out[f"samespeaker_offset{offset}"] = _artefacts(seqLabel, W, ref_ds.SameSpeakerSampler(4, speakerLabel, W, offset))
        torch.manual_seed(6 + offset)
        out[f"temporal_offset{offset}"] = _artefacts(seqLabel, W, ref_ds.TemporalSameSpeakerSampler(3, speakerLabel, W, offset))
    # hand-made batches: inside a sequence, over a boundary, over the end of the last sequence (not last / last of its batch),
    # an offset beyond the last boundary, a negative offset, a window that ends exactly on a boundary, and the carried shift
    hand = [[0, 100, 150], [200, 500, 601], [1850, 1901, 300], [300, 1950], [2000, 2500, 20], [-5, 40], [150, 900], [1899, 0]]
    for temporal in (False, True):
        sampler = ref_ds.TemporalSameSpeakerSampler(3, speakerLabel, W, 0) if temporal else ref_ds.SameSpeakerSampler(4, speakerLabel, W, 0)
        sampler.batches = [list(b) for b in hand]
        out["hand_temporal" if temporal else "hand_independent"] = _artefacts(seqLabel, W, sampler)
    carried = ref_ds.TemporalSameSpeakerSampler(3, speakerLabel, W, 0)
    carried.batches = [[180, 280, 380, 480], [520, 620, 720], [1700, 1800, 1900], [1750, 1850, 1950]]
    out["hand_carried_shift"] = _artefacts(seqLabel, W, carried)
    return out


# ----------------------------------------------------------------------------- the lists main builds
class _Recorded(Exception):
    pass


def _lists_of_main(argv):
    calls = []

    def recorder(path, sizeWindow, seqNames, *a, **k):
        calls.append([list(s) for s in seqNames])
        if len(calls) == 2:
            raise _Recorded()

    saved = ref_train.AudioBatchData
    ref_train.AudioBatchData = recorder
    try:
        quiet(ref_train.main, list(argv))
    except _Recorded:
        pass
    finally:
        ref_train.AudioBatchData = saved
    return calls


def record_split():
    out = {}
    cache_dir = tempfile.mkdtemp(prefix="g23_split_")
    _, speakers = quiet(ref_ds.findAllSeqs, DB, extension=".flac", cache_path=os.path.join(cache_dir, "plain.txt"))
    base = ["--pathDB", "tests/golden/test_db", "--nGPU", "0"]

    def run(tag, extra, seed, names):
        argv = base + extra + ["--random_seed", str(seed), "--path_cache", os.path.join(cache_dir, f"{tag}_{seed}.txt")]
        train, val = _lists_of_main(argv)
        return {"argv": base + extra + ["--random_seed", str(seed)], "seed": seed,
                "train": [[names[i], rel] for i, rel in train], "val": [[names[i], rel] for i, rel in val]}

    out["path_train"] = [run("path_train", ["--pathTrain", "tests/golden/seq_list.txt"], seed, speakers) for seed in (0, 1)]
    temporal = ["--samplingType", "temporalsamespeaker", "--naming_convention", "spkr-id"]
    _, ids = quiet(ref_ds.findAllSeqs, DB, extension=".flac", format="spkr-id", cache_path=os.path.join(cache_dir, "ids.txt"))
    per_speaker = {}
    for rel in (os.path.join(r, f)[len(DB) + 1:] for r, _d, fs in os.walk(DB) for f in fs if f.endswith(".flac")):
        per_speaker[rel.split(os.sep)[0]] = per_speaker.get(rel.split(os.sep)[0], 0) + 1
    found = []
    for seed in range(64):
        entry = run("temporal", temporal, seed, ids)
        (val_name, val_rel), = entry["val"]
        if per_speaker[val_rel.split(os.sep)[0]] == 1:
            found.append(entry)
        if len(found) == 2:
            break
    out["temporal_spkr_id"] = found
    return out


def main():
    random.seed(0)
    data = {"parse": record_parse(), "find": record_find(), "artefacts": record_artefacts(), "split": record_split()}
    with open(OUT, "w") as fh:
        json.dump(data, fh, indent=1, sort_keys=True)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
