"""The training command line (cpc2_amd.train.parseArgs / main, cpc2_amd.cpc_default_config) and what it exposes in the
feeder (naming conventions, sequence cache, remove_artefacts) and the optimiser (FlatSGD's state dict), without a GPU.

tests/golden/g23_train_cli.json holds what the reference answers (tools/make_golden_train_cli.py).  Speaker INDICES follow
os.walk order, which differs from box to box: sequences are compared with their speaker NAME.  Under the spkr-id convention
tests/golden/test_db holds files with equal sort keys (same speaker and chapter); a sort keeps those in os.walk order, so
the lists of that case are compared after ordering the files INSIDE a run of equal keys by name -- every other position is
compared as recorded."""
import json
import os
import random

import pytest
import torch

from cpc2_amd import dataset as ds
from cpc2_amd import train as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DB = os.path.join(ROOT, "tests", "golden", "test_db")
SEQ_LIST = os.path.join(ROOT, "tests", "golden", "seq_list.txt")
with open(os.path.join(ROOT, "tests", "golden", "g23_train_cli.json")) as _fh:
    G23 = json.load(_fh)


# ----------------------------------------------------------------------------- parseArgs
@pytest.mark.parametrize("tag", sorted(G23["parse"]))
def test_parse_args_equal_the_reference(tag, monkeypatch, capsys):
    monkeypatch.chdir(ROOT)
    entry = G23["parse"][tag]
    args = tr.parseArgs(list(entry["argv"]))
    want = json.loads(json.dumps(entry["args"]).replace("$ROOT", ROOT))
    got = json.loads(json.dumps(vars(args)))
    assert "--nGPU" in entry["argv"]                 # (every recorded command line pins it: nothing is excluded)
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}
    assert len(got) == 82


def test_default_config_alone_has_the_reference_keys():
    from cpc2_amd.cpc_default_config import get_default_cpc_config
    cfg = vars(get_default_cpc_config())
    own = {"pathDB", "file_extension", "pathTrain", "pathVal", "n_process_loader", "ignore_cache", "path_cache",
           "max_size_loaded", "supervised", "pathPhone", "CTC", "pathCheckpoint", "logging_step", "save_step", "load",
           "loadCriterion", "restart", "nGPU", "batchSizeGPU", "debug", "distributed", "local_rank", "master_port"}
    want = G23["parse"]["defaults"]["args"]
    assert set(cfg) == set(want) - own
    for key, value in cfg.items():
        if key != "random_seed":
            assert value == want[key], key
    # ... which are the keys a reference run wrote into its checkpoint_args.json
    with open(os.path.join(ROOT, "tests", "golden", "ref_checkpoint", "checkpoint_args.json")) as fh:
        assert set(cfg) <= set(json.load(fh))


def test_parse_args_draws_a_seed_and_resolves_ngpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 3)
    args = tr.parseArgs(["--pathDB", "db"])
    assert args.nGPU == 3 and isinstance(args.random_seed, int) and 0 <= args.random_seed <= 2 ** 31
    with pytest.raises(AssertionError):
        tr.parseArgs(["--pathDB", "db", "--nGPU", "4"])


@pytest.mark.parametrize("argv", [
    ["--pathDB", "db", "--samplingType", "temporalsamespeaker", "--naming_convention", "spkr-id", "--pathTrain", "x.txt"],
    ["--pathDB", "db", "--samplingType", "temporalsamespeaker", "--naming_convention", "spkr-id", "--pathVal", "x.txt"],
    ["--pathDB", "db", "--samplingType", "temporalsamespeaker"],
    ["--pathDB", "db", "--meta_aug_type", "natural_reverb"],
    ["--pathDB", "db", "--meta_aug"],
])
def test_parse_args_value_errors(argv):
    with pytest.raises(ValueError):
        tr.parseArgs(argv + ["--nGPU", "0"])


@pytest.mark.parametrize("argv", [[], ["--pathCheckpoint", "somewhere", "--restart"], ["--nGPU", "0"]])
def test_parse_args_prints_help_and_exits_without_data_or_checkpoint(argv, capsys):
    with pytest.raises(SystemExit):
        tr.parseArgs(argv)
    out = capsys.readouterr().out
    assert "--pathDB" in out and "Either provides an input dataset or a checkpoint to load" in out


# ----------------------------------------------------------------------------- refusals
MISSING = os.path.join(ROOT, "tests", "golden", "no_such_data_set")
REFUSED = [
    (["--augment_past", "--augment_type", "pitch"], NotImplementedError, "--augment_past"),
    (["--augment_future", "--augment_type", "additive", "bandreject"], NotImplementedError, "--augment_future"),
    (["--encoder_type", "mfcc"], NotImplementedError, "--encoder_type mfcc"),
    (["--encoder_type", "lfb"], NotImplementedError, "--encoder_type lfb"),
    (["--cpc_mode", "bert"], NotImplementedError, "--cpc_mode bert"),
    (["--normMode", "batchNorm"], NotImplementedError, "--normMode batchNorm"),
    (["--normMode", "instanceNorm"], NotImplementedError, "--normMode instanceNorm"),
    (["--normMode", "ID"], NotImplementedError, "--normMode ID"),
    (["--rnnMode", "ffd"], NotImplementedError, "--rnnMode ffd"),
    (["--rnnMode", "conv4"], NotImplementedError, "--rnnMode conv4"),
    (["--rnnMode", "conv8"], NotImplementedError, "--rnnMode conv8"),
    (["--rnnMode", "conv12"], NotImplementedError, "--rnnMode conv12"),
    (["--rnnMode", "transformer_adaptive_span"], NotImplementedError, "--rnnMode transformer_adaptive_span"),
    (["--rnnMode", "linear", "--multihead_rnn"], NotImplementedError, "--multihead_rnn"),
    (["--supervised"], NotImplementedError, "linear_separability --unfrozen"),
    (["--supervised", "--pathPhone", "phones.txt", "--CTC"], NotImplementedError, "--supervised"),
]


@pytest.mark.parametrize("flags,error,text", REFUSED, ids=[" ".join(r[0]) for r in REFUSED])
def test_main_refuses_before_the_data_set_is_opened(flags, error, text, monkeypatch):
    opened = []
    monkeypatch.setattr(ds, "findAllSeqs", lambda *a, **k: opened.append(a) or ([], []))
    with pytest.raises(error, match=text):
        tr.main(["--pathDB", MISSING, "--nGPU", "0", "--random_seed", "0"] + flags)
    assert not opened and not os.path.exists(MISSING)


def test_main_refuses_several_gpus_in_one_process(monkeypatch):
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 8)
    for argv in (["--nGPU", "2"], []):               # asked for, or resolved from the device count
        with pytest.raises(SystemExit, match="--nGPU .* --distributed"):
            tr.main(["--pathDB", MISSING, "--random_seed", "0"] + argv)


def test_get_criterion_still_refuses_supervised_and_points_to_the_probe():
    import types
    with pytest.raises(NotImplementedError, match="linear_separability --unfrozen"):
        tr.getCriterion(types.SimpleNamespace(supervised=True), 160)


def test_main_says_when_there_is_no_validation_data(monkeypatch, tmp_path):
    """(the reference builds no validation set and fails inside its epoch loop)"""
    def no_dataset(*a, **k):
        raise AssertionError("a data set was loaded")
    monkeypatch.setattr(ds, "AudioBatchData", no_dataset)
    monkeypatch.setattr(ds, "findAllSeqs", lambda *a, **k: ([(0, "a/one.flac"), (0, "a/two.flac")], ["a"]))
    (tmp_path / "train.txt").write_text("one\ntwo\n")
    (tmp_path / "val.txt").write_text("three\n")
    base = ["--pathDB", str(tmp_path), "--nGPU", "0", "--random_seed", "0", "--path_cache", str(tmp_path / "c.txt")]
    with pytest.raises(ValueError, match="No validation"):
        tr.main(base + ["--pathTrain", str(tmp_path / "train.txt"), "--pathVal", str(tmp_path / "val.txt")])
    with pytest.raises(ValueError, match="No training"):
        tr.main(base + ["--pathTrain", str(tmp_path / "val.txt")])
    monkeypatch.setattr(ds, "findAllSeqs", lambda *a, **k: ([(0, "a/one.flac")], ["a"]))
    with pytest.raises(ValueError, match="No training"):           # one file: the split sends it to validation
        tr.main(base)


# ----------------------------------------------------------------------------- findAllSeqs
def _make_tree(base, names):
    for rel in names:
        path = base / rel
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_bytes(b"")


@pytest.mark.parametrize("no_speaker", [False, True], ids=["speaker", "no_speaker"])
@pytest.mark.parametrize("convention", sorted(G23["find"]))
def test_find_all_seqs_naming_conventions(convention, no_speaker, tmp_path, capsys):
    entry = G23["find"][convention]
    _make_tree(tmp_path, entry["files"])
    seqs, speakers = ds.findAllSeqs(str(tmp_path), no_speaker=no_speaker, extension=".flac", format=convention)
    want = entry["no_speaker" if no_speaker else "speaker"]
    assert [[speakers[i], rel] for i, rel in seqs] == want["seqs"]
    assert sorted(speakers) == want["speakers"]
    assert not (tmp_path / "_seqs_cache.txt").exists()                 # no cache argument: no file


def test_find_all_seqs_unknown_convention(tmp_path):
    _make_tree(tmp_path, ["a/x_1.flac"])
    with pytest.raises(ValueError, match="format unknown"):
        ds.findAllSeqs(str(tmp_path), format="by-moon-phase")


def test_find_all_seqs_plain_call_is_unchanged_and_leaves_no_file():
    before = sorted(os.listdir(DB))
    seqs, speakers = ds.findAllSeqs(DB, extension=".flac")
    assert sorted(os.listdir(DB)) == before
    assert len(seqs) == 9 and sorted(speakers) == ["2911", "4051", "4397", "5393", "5678", "6476"]
    assert all(rel.split(os.sep)[0] == speakers[i] for i, rel in seqs)
    # os.walk order, as before the conventions existed
    walked = [os.path.relpath(os.path.join(r, f), DB) for r, _d, fs in os.walk(DB + os.sep, followlinks=True)
              for f in fs if f.endswith(".flac")]
    assert [rel for _, rel in seqs] == walked


def test_find_all_seqs_cache_round_trip(tmp_path, capsys):
    _make_tree(tmp_path / "db", G23["find"]["spkr-id"]["files"])
    db, cache = str(tmp_path / "db"), str(tmp_path / "cache" / "seqs.txt")
    (tmp_path / "cache").mkdir()
    first = ds.findAllSeqs(db, format="spkr-id", loadCache=True, cache_path=cache)     # nothing to load: rebuilt, saved
    out = capsys.readouterr().out
    assert "Could not load cache, rebuilding" in out and f"Saved cache file at {cache}" in out and os.path.exists(cache)
    (tmp_path / "db" / "9" / "9").mkdir(parents=True)
    (tmp_path / "db" / "9" / "9" / "9-9-0001.flac").write_bytes(b"")
    cached = ds.findAllSeqs(db, format="spkr-id", loadCache=True, cache_path=cache)
    assert f"Loaded from cache {cache} successfully" in capsys.readouterr().out
    assert (list(map(tuple, cached[0])), cached[1]) == (list(map(tuple, first[0])), first[1])     # keyed by nothing: the stale list
    fresh = ds.findAllSeqs(db, format="spkr-id", loadCache=False, cache_path=cache)    # --ignore_cache: rebuilt AND overwritten
    assert len(fresh[0]) == len(first[0]) + 1
    assert len(ds.findAllSeqs(db, format="no_speaker", loadCache=True, cache_path=cache)[0]) == len(fresh[0])
    # default location: inside the data set
    ds.findAllSeqs(db, format="spkr-id", loadCache=True)
    assert os.path.exists(os.path.join(db, "_seqs_cache.txt"))
    # a directory that cannot be written to is tolerated
    gone = str(tmp_path / "not_there" / "seqs.txt")
    seqs, _ = ds.findAllSeqs(db, format="spkr-id", loadCache=True, cache_path=gone)
    out = capsys.readouterr().out
    assert "Ran in an error while loading" in out and "Ran in an error while saving" in out and len(seqs) == len(fresh[0])


# ----------------------------------------------------------------------------- remove_artefacts
@pytest.mark.parametrize("tag", sorted(G23["artefacts"]))
def test_remove_artefacts_equals_the_reference(tag):
    case = G23["artefacts"][tag]
    got = ds.remove_artefacts([list(b) for b in case["before"]], case["seqLabel"], case["sizeWindow"],
                              carry_shift=case["temporal"])
    assert got == case["after"]
    assert case["before"] != case["after"]                              # (every recorded case moves or drops something)


def test_remove_artefacts_bisection_equals_the_walk_on_random_tables():
    """The independent (searchsorted) and the carried (bisect) form against a restatement of the boundary walk."""
    rng = random.Random(3)
    for _ in range(50):
        bounds = [0]
        for _n in range(rng.randint(1, 9)):
            bounds.append(bounds[-1] + rng.randint(0, 400))
        w = rng.randint(1, 150)
        batches = [[rng.randint(-50, bounds[-1] + 50) for _i in range(rng.randint(1, 6))] for _b in range(8)]
        for carry in (False, True):
            want = []
            for batch in batches:
                new, shift, delete = [], 0, False
                for beg in batch:
                    beg += shift
                    delete = False
                    for i in range(1, len(bounds)):
                        if bounds[i - 1] <= beg < bounds[i]:
                            if beg + w > bounds[i]:
                                if i != len(bounds) - 1:
                                    new.append(bounds[i])
                                else:
                                    delete = True
                                if carry:
                                    shift += bounds[i] - beg
                            else:
                                new.append(beg)
                if not delete:
                    want.append(new)
            assert ds.remove_artefacts(batches, bounds, w, carry_shift=carry) == want


def _cpu_dataset(window=2048):
    seqs, speakers = ds.findAllSeqs(DB, extension=".flac")
    seqs = sorted(ds.filterSeqs(SEQ_LIST, seqs), key=lambda s: s[1])
    random.seed(0)
    return ds.AudioBatchData(DB, window, seqs, None, len(speakers), device="cpu")


def _offsets_of(loader, data):
    """The window offsets a CPU loader yields, recovered through AudioBatchData.windows."""
    seen = []
    original = data.windows
    data.windows = lambda offsets: seen.append(list(offsets)) or original(offsets)
    try:
        batches = [(x.clone(), y.clone()) for x, y in loader]
    finally:
        del data.windows
    return seen, batches


@pytest.mark.parametrize("sampling,batch", [("samespeaker", 8), ("uniform", 8), ("temporalsamespeaker", 2)])
def test_loader_with_remove_artefacts_never_crosses_a_sequence_boundary(sampling, batch):
    import bisect
    data = _cpu_dataset()
    crossing_before = 0
    for seed in range(3):
        for flag in (False, True):
            random.seed(seed)
            torch.manual_seed(seed)
            offsets, _ = _offsets_of(data.getDataLoader(batch, sampling, True, remove_artefacts=flag), data)
            assert offsets
            crossing = sum(1 for b in offsets for o in b
                           if o + data.sizeWindow > data.seqLabel[bisect.bisect_right(data.seqLabel, o)])
            if flag:
                assert crossing == 0
            else:
                crossing_before += crossing
    assert crossing_before > 0                       # (the plain loader does cross: the flag has something to do)


@pytest.mark.parametrize("sampling", ["samespeaker", "uniform", "sequential", "temporalsamespeaker"])
def test_default_loader_is_unchanged_by_the_new_arguments(sampling):
    data = _cpu_dataset()
    runs = []
    for kwargs in ({}, {"remove_artefacts": False, "batch_size_per_gpu": 4}):
        random.seed(7)
        torch.manual_seed(7)
        runs.append(_offsets_of(data.getDataLoader(4, sampling, True, **kwargs), data))
    (off_a, bat_a), (off_b, bat_b) = runs
    assert off_a == off_b and len(bat_a) == len(bat_b) > 0
    assert all(torch.equal(xa, xb) and torch.equal(ya, yb) for (xa, ya), (xb, yb) in zip(bat_a, bat_b))
    # ... and is what the samplers give for that seed (nothing else draws)
    random.seed(7)
    torch.manual_seed(7)
    offset = random.randint(0, data.sizeWindow * 4) if sampling == "temporalsamespeaker" else random.randint(0, data.sizeWindow // 2)
    limit = data.data.numel() - data.sizeWindow
    want = [[o for o in b if 0 <= o <= limit] for b in data.getBaseSampler(sampling, 4, offset)]
    assert off_a == [b for b in want if b]


# ----------------------------------------------------------------------------- the lists main builds
class _Recorded(Exception):
    pass


def _lists_of_main(argv, monkeypatch, tmp_path):
    calls = []

    def recorder(path, sizeWindow, seqNames, phoneLabels, nSpeakers, **kwargs):
        calls.append(([list(s) for s in seqNames], nSpeakers, kwargs))
        if len(calls) == 2:
            raise _Recorded()

    monkeypatch.setattr(ds, "AudioBatchData", recorder)
    monkeypatch.chdir(ROOT)
    with pytest.raises(_Recorded):
        tr.main(list(argv) + ["--path_cache", str(tmp_path / "cache.txt")])
    return calls


def _tie_groups_by_name(named, key):
    """Order the files inside every run of equal sort key by name (see the module docstring)."""
    out, i = [], 0
    while i < len(named):
        j = i
        while j < len(named) and key(named[j][1]) == key(named[i][1]):
            j += 1
        out.extend(sorted(named[i:j], key=lambda item: item[1]))
        i = j
    return out


@pytest.mark.parametrize("case", range(2))
def test_main_train_and_validation_lists_with_path_train(case, monkeypatch, tmp_path, capsys):
    entry = G23["split"]["path_train"][case]
    _, speakers = ds.findAllSeqs(DB, extension=".flac")
    (train, n_spk, kw_train), (val, _n, kw_val) = _lists_of_main(entry["argv"], monkeypatch, tmp_path)
    assert [[speakers[i], rel] for i, rel in train] == entry["train"]
    assert [[speakers[i], rel] for i, rel in val] == entry["val"]
    assert n_spk == 6 and kw_train["keep_temporality"] is False and kw_train["MAX_SIZE_LOADED"] == 4000000000
    assert not os.path.exists(os.path.join(DB, "_seqs_cache.txt"))


@pytest.mark.parametrize("case", range(2))
def test_main_train_and_validation_lists_temporal_spkr_id(case, monkeypatch, tmp_path, capsys):
    entry = G23["split"]["temporal_spkr_id"][case]
    _, ids = ds.findAllSeqs(DB, extension=".flac", format="spkr-id")
    (train, n_spk, kw_train), (val, _n, _kw) = _lists_of_main(entry["argv"], monkeypatch, tmp_path)

    def key(rel):
        return rel.split('-')[0], int(rel.split('-')[1])
    got_train = _tie_groups_by_name([[ids[i], rel] for i, rel in train], key)
    assert got_train == _tie_groups_by_name(entry["train"], key)
    assert [[ids[i], rel] for i, rel in val] == entry["val"]
    assert n_spk == len(ids) == 7 and kw_train["keep_temporality"] is True
    # a speaker's files stay together and in order
    seen = []
    for i, _rel in train:
        if not seen or seen[-1] != i:
            assert i not in seen
            seen.append(i)


def test_split_keeps_95_percent_and_blocks(monkeypatch):
    seqs = [(i // 3, f"f{i}") for i in range(40)]
    random.seed(1)
    train, val = tr.splitTrainVal(seqs, "samespeaker")
    assert len(train) == 38 and len(val) == 2 and sorted(train + val) == sorted(seqs) and train + val != seqs
    random.seed(1)
    train, val = tr.splitTrainVal(seqs, "temporalsamespeaker")
    joined = train + val
    assert sorted(joined) == sorted(seqs) and joined != seqs
    for spk in range(14):
        names = [n for s, n in joined if s == spk]
        assert names == [n for s, n in seqs if s == spk]
        where = [k for k, (s, _n) in enumerate(joined) if s == spk]
        assert where == list(range(where[0], where[0] + len(where)))


def test_set_seed_seeds_every_generator():
    import numpy as np
    tr.set_seed(5)
    a = (random.random(), float(torch.rand(1)), float(np.random.rand()))
    tr.set_seed(5)
    assert a == (random.random(), float(torch.rand(1)), float(np.random.rand()))


# ----------------------------------------------------------------------------- FlatSGD's state dict
def _flat_sgd_on_cpu(params, monkeypatch):
    """FlatSGD's bookkeeping without a device: only the GPU requirement of the constructor is lifted; step() is not called."""
    from cpc2_amd import _lib
    monkeypatch.setattr(_lib, "require_gpu", lambda *a, **k: None)
    return tr.FlatSGD(params, lr=0.05)


def test_flat_sgd_state_dict_round_trips_through_torch_sgd(monkeypatch):
    shapes = [(3, 4), (5,), (2, 2, 2)]
    torch.manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(s)) for s in shapes]
    opt = _flat_sgd_on_cpu(params, monkeypatch)
    assert opt.state_dict()["state"] == {}                             # before the first step: as torch.optim.SGD
    torch.optim.SGD([torch.nn.Parameter(torch.zeros(s)) for s in shapes], lr=1.0, momentum=0.9).load_state_dict(opt.state_dict())
    opt.momentum_buffer.copy_(torch.arange(opt.momentum_buffer.numel(), dtype=torch.float32))
    opt.step_count = 2
    opt.param_groups[0]["initial_lr"] = 0.2
    sd = opt.state_dict()
    theirs = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    ref = torch.optim.SGD(theirs, lr=1.0, momentum=0.9)
    ref.load_state_dict(sd)
    assert ref.param_groups[0]["lr"] == 0.05 and ref.param_groups[0]["momentum"] == 0.9
    assert ref.param_groups[0]["initial_lr"] == 0.2
    off = 0
    for p, s in zip(theirs, shapes):
        buf = ref.state[p]["momentum_buffer"]
        assert tuple(buf.shape) == s and torch.equal(buf.reshape(-1), torch.arange(off, off + buf.numel(), dtype=torch.float32))
        off += buf.numel()
    # torch's own step accepts the loaded state: buf = 0.9 buf + g, p -= lr buf
    for p in theirs:
        p.grad = torch.ones_like(p)
    ref.step()
    assert torch.allclose(theirs[1].detach(), -0.05 * (0.9 * torch.arange(12, 17, dtype=torch.float32) + 1))
    # and back
    back = _flat_sgd_on_cpu([torch.nn.Parameter(torch.zeros(s)) for s in shapes], monkeypatch)
    back.load_state_dict(ref.state_dict())
    want = torch.cat([ref.state[p]["momentum_buffer"].reshape(-1) for p in theirs])
    assert torch.equal(back.momentum_buffer, want) and back.step_count >= 1
    assert back.param_groups[0]["lr"] == 0.05 and back.param_groups[0]["initial_lr"] == 0.2
    back.load_state_dict({"state": {}, "param_groups": [{"lr": 0.1}]})                  # no buffers: a first step comes next
    assert back.step_count == 0 and float(back.momentum_buffer.abs().sum()) == 0


def test_build_optimizer_chooses_by_name(monkeypatch):
    from cpc2_amd import _lib
    monkeypatch.setattr(_lib, "require_gpu", lambda *a, **k: None)
    model, crit = torch.nn.Linear(3, 2), torch.nn.Linear(2, 1)
    assert type(tr.buildOptimizer(model, crit)) is tr.FlatAdam
    model, crit = torch.nn.Linear(3, 2), torch.nn.Linear(2, 1)
    sgd = tr.buildOptimizer(model, crit, lr=0.3, optimizer="sgd")
    assert type(sgd) is tr.FlatSGD and sgd.momentum == 0.9 and sgd.param_groups[0]["lr"] == 0.3
    assert sgd.params[0] is crit.weight                                 # criterion parameters first
    with pytest.raises(ValueError, match="Unsupported optimizer"):
        tr.buildOptimizer(model, crit, optimizer="lion")


def test_flat_adam_state_dict_carries_initial_lr(monkeypatch):
    """A scheduler built on a resumed optimiser takes its base rate from the group's initial_lr."""
    from cpc2_amd import _lib
    monkeypatch.setattr(_lib, "require_gpu", lambda *a, **k: None)
    first = tr.FlatAdam([torch.nn.Parameter(torch.zeros(4))], lr=1e-3)
    assert "initial_lr" not in first.state_dict()["param_groups"][0]
    sched = tr.buildScheduler(first, schedulerRamp=5)
    for _ in range(3):
        sched.step()                                                    # three epochs done: the rate is 4/5 of the base
    sd = first.state_dict()
    assert sd["param_groups"][0]["initial_lr"] == 1e-3 and abs(sd["param_groups"][0]["lr"] - 0.8e-3) < 1e-12
    resumed = tr.FlatAdam([torch.nn.Parameter(torch.zeros(4))], lr=5e-2)
    resumed.load_state_dict(sd)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sched = tr.buildScheduler(resumed, schedulerRamp=5, epochs_done=3)
    assert abs(resumed.param_groups[0]["lr"] - 0.8e-3) < 1e-12
    sched.step()
    assert abs(resumed.param_groups[0]["lr"] - 1e-3) < 1e-12
    # torch.optim.Adam reads the same dict
    ref = torch.optim.Adam([torch.nn.Parameter(torch.zeros(4))], lr=1.0)
    ref.load_state_dict(sd)
    assert ref.param_groups[0]["initial_lr"] == 1e-3
