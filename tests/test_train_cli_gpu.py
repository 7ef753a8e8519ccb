"""`python -m cpc2_amd.train` end to end on the GPU: cpc2_amd.train.main on tests/golden/test_db at a small width (seconds per
run), its files, equality with the loop assembled by hand, resume (schedule, optimiser state, a reference-written
checkpoint), --optimizer sgd (FlatSGD / cpc_sgd_step against an fp64 statement of the rule), --no_artefacts, and the module
entry point as a child process.  Every run of main gets a --path_cache of its own (the sequence cache is keyed by nothing)."""
import json
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import cpc2_amd
from cpc2_amd import _lib
from cpc2_amd import dataset as ds
from cpc2_amd import feature_loader as fl
from cpc2_amd import train as tr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DB = os.path.join(ROOT, "tests", "golden", "test_db")
SEQ_LIST = os.path.join(ROOT, "tests", "golden", "seq_list.txt")
REF_CKPT = os.path.join(ROOT, "tests", "golden", "ref_checkpoint")
DEV = "cuda:0"
SMALL = ["--hiddenEncoder", "64", "--hiddenGar", "64", "--nPredicts", "4", "--negativeSamplingExt", "16", "--arMode", "GRU",
         "--rnnMode", "linear", "--batchSizeGPU", "8", "--nGPU", "1", "--random_seed", "0", "--save_step", "1"]
LISTS = ["--pathTrain", SEQ_LIST, "--pathVal", SEQ_LIST]           # (takes the split's shuffle out of the runs that are compared)


def rel_err(got, ref):
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((g - r).abs().max() / (r.abs().max() + 1e-30))


def assert_close(got, ref, tol, what="", rtol=None):
    """tests/test_gpu_parity.py's check, restated: |got - ref|_inf <= tol * |ref|_inf AND, element by element,
    |got - ref| <= atol + rtol * |ref| with atol = tol * |ref|_inf and rtol = 64 * tol."""
    e = rel_err(got, ref)
    assert e <= tol, f"{what}: rel err {e:.3e} > {tol:.1e}"
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    atol = tol * float(r.abs().max()) + 1e-30
    rt = 64 * tol if rtol is None else rtol
    bad = (g - r).abs() > atol + rt * r.abs()
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements outside atol {atol:.2e} + {rt:.1e} |ref|"


_TRAIN_STEP = tr.trainStep


def _argv(out_dir, *extra, lists=True):
    os.makedirs(out_dir, exist_ok=True)
    return (["--pathDB", DB, "--pathCheckpoint", os.path.join(out_dir, "run"), "--path_cache", os.path.join(out_dir, "seqs_cache.txt")]
            + SMALL + (LISTS if lists else []) + list(extra))


def _watch(monkeypatch):
    """Record, at the start of every trainStep, the learning rate, the optimiser's step count and (first call) a snapshot."""
    seen = {"lr": [], "step_count": [], "first": None}
    original = _TRAIN_STEP

    def watched(loader, model, criterion, optimizer, *a, **k):
        seen["lr"].append(optimizer.param_groups[0]["lr"])
        seen["step_count"].append(optimizer.step_count)
        if seen["first"] is None:
            seen["first"] = {"model": {n: v.detach().cpu().clone() for n, v in model.state_dict().items()},
                             "criterion": {n: v.detach().cpu().clone() for n, v in criterion.state_dict().items()},
                             "optimizer": optimizer.state_dict()}
        return original(loader, model, criterion, optimizer, *a, **k)

    monkeypatch.setattr(tr, "trainStep", watched)
    return seen


def _finite(values):
    return all(np.isfinite(np.asarray(v, dtype=np.float64)).all() for v in values)


def _run_files(run_dir, epochs):
    names = set(os.listdir(run_dir))
    assert {"checkpoint_args.json", "checkpoint_logs.json"} <= names, names
    for e in epochs:
        assert f"checkpoint_{e}.pt" in names, names
    with open(os.path.join(run_dir, "checkpoint_logs.json")) as fh:
        return json.load(fh)


# ----------------------------------------------------------------------------- 1. three epochs, the files
def test_main_three_epochs_writes_the_reference_layout(tmp_path, capsys):
    argv = _argv(str(tmp_path), "--nEpoch", "3")
    res = tr.main(argv)
    run_dir = str(tmp_path / "run")
    logs = _run_files(run_dir, [0, 1, 2])
    assert logs["epoch"] == [0, 1, 2] and logs["saveStep"] == 1 and logs["logging_step"] == 1000
    for key in ("locLoss_train", "locAcc_train", "locLoss_val", "locAcc_val"):
        assert len(logs[key]) == 3 and all(len(v) == 4 for v in logs[key]) and _finite(logs[key]), key
    with open(os.path.join(run_dir, "checkpoint_args.json")) as fh:
        written = json.load(fh)
    assert set(written) == set(vars(tr.parseArgs(argv))) | {"is_local_master"}
    assert written["is_local_master"] is True and written["pathCheckpoint"] == os.path.join(run_dir, "checkpoint")
    for e in range(3):
        ckpt = torch.load(os.path.join(run_dir, f"checkpoint_{e}.pt"), "cpu")
        assert set(ckpt) == {"gEncoder", "cpcCriterion", "optimizer", "best"}
    # loadModel on the last one gives the features of the in-memory model, bit for bit
    loaded, hidden_gar, hidden_enc = fl.loadModel([os.path.join(run_dir, "checkpoint_2.pt")])
    assert (hidden_gar, hidden_enc) == (64, 64)
    loaded = loaded.to(DEV).eval()
    res.cpcModel.eval()
    torch.manual_seed(3)
    x = torch.randn(3, 1, 20480, device=DEV) * 0.1
    with torch.no_grad():
        c_mem, z_mem, _ = res.cpcModel(x, None)
        c_new, z_new, _ = loaded(x, None)
    assert torch.equal(c_mem, c_new) and torch.equal(z_mem, z_new)
    assert not os.path.exists(os.path.join(DB, "_seqs_cache.txt"))


# ----------------------------------------------------------------------------- 2. main adds nothing to the loop
def test_main_equals_the_loop_assembled_by_hand(tmp_path, capsys):
    argv = _argv(str(tmp_path / "main"), "--nEpoch", "3")
    res = tr.main(argv)
    # the same pieces by hand, drawing from the generators in main's order: seed, the two data sets, the modules
    args = tr.parseArgs(_argv(str(tmp_path / "hand"), "--nEpoch", "3"))
    tr.set_seed(args.random_seed)
    seqs, speakers = ds.findAllSeqs(DB, extension=".flac")
    train = ds.AudioBatchData(DB, args.sizeWindow, ds.filterSeqs(SEQ_LIST, seqs), None, len(speakers), keep_temporality=False,
                              device=DEV)
    val = ds.AudioBatchData(DB, args.sizeWindow, ds.filterSeqs(SEQ_LIST, seqs), None, len(speakers), device=DEV)
    model = cpc2_amd.CPCModel(tr.getEncoder(args), tr.getAR(args), args.mask_prob, args.mask_length)
    crit = tr.getCriterion(args, model.gEncoder.DOWNSAMPLING, len(speakers), None)
    crit.to(DEV)
    model.to(DEV)
    opt = tr.buildOptimizer(model, crit, lr=args.learningRate, beta1=args.beta1, beta2=args.beta2, epsilon=args.epsilon)
    os.makedirs(args.pathCheckpoint, exist_ok=True)
    ckpt = os.path.join(args.pathCheckpoint, "checkpoint")
    with open(ckpt + "_args.json", "w") as fh:
        json.dump(vars(args), fh)
    logs = {"epoch": [], "iter": [], "saveStep": args.save_step, "logging_step": args.logging_step}
    tr.run(train, val, args.batchSizeGPU, args.samplingType, model, crit, args.nEpoch, ckpt, opt, None, logs)
    assert opt.flat.numel() == res.optimizer.flat.numel() and opt.step_count == res.optimizer.step_count > 0
    assert torch.equal(opt.flat, res.optimizer.flat), "parameters"
    assert torch.equal(opt.exp_avg, res.optimizer.exp_avg) and torch.equal(opt.exp_avg_sq, res.optimizer.exp_avg_sq)
    assert json.dumps(logs, sort_keys=True) == json.dumps(res.logs, sort_keys=True)
    a = torch.load(os.path.join(str(tmp_path / "main" / "run"), "checkpoint_2.pt"), "cpu")
    b = torch.load(ckpt + "_2.pt", "cpu")
    for part in ("gEncoder", "cpcCriterion"):
        assert list(a[part]) == list(b[part]) and all(torch.equal(a[part][k], b[part][k]) for k in a[part]), part


# ----------------------------------------------------------------------------- 3. resume
def test_resume_continues_schedule_and_optimizer_and_restart_does_not(tmp_path, monkeypatch, capsys):
    lr0 = 1e-3
    first_dir, whole_dir = str(tmp_path / "stopped"), str(tmp_path / "whole")
    seen = _watch(monkeypatch)
    tr.main(_argv(first_dir, "--nEpoch", "3", "--schedulerRamp", "5", "--learningRate", str(lr0)))
    assert seen["lr"] == [lr0 * tr.ramp_scheduling_function(5, e) for e in range(3)]
    saved = torch.load(os.path.join(first_dir, "run", "checkpoint_2.pt"), "cpu")["optimizer"]
    saved_step = int(saved["state"][0]["step"])
    assert saved_step > 0 and saved["param_groups"][0]["initial_lr"] == lr0

    resumed = _watch(monkeypatch)
    res = tr.main(_argv(first_dir, "--nEpoch", "5", "--learningRate", "0.05"))
    assert res.logs["epoch"] == [0, 1, 2, 3, 4] and len(resumed["lr"]) == 2             # started at epoch 3
    assert res.args.nEpoch == 5 and res.args.learningRate == lr0 and res.args.schedulerRamp == 5
    assert resumed["step_count"][0] == saved_step                                       # Adam's step count continues
    assert res.optimizer.step_count > resumed["step_count"][1] > saved_step
    restored = resumed["first"]["optimizer"]["state"]
    assert all(torch.equal(restored[i]["exp_avg"].cpu(), saved["state"][i]["exp_avg"]) for i in saved["state"])
    assert resumed["lr"] == [lr0 * tr.ramp_scheduling_function(5, e) for e in (3, 4)]

    whole = _watch(monkeypatch)
    tr.main(_argv(whole_dir, "--nEpoch", "5", "--schedulerRamp", "5", "--learningRate", str(lr0)))
    assert len(whole["lr"]) == 5 and whole["lr"][3:] == resumed["lr"]                   # what an uninterrupted run has there
    _run_files(os.path.join(first_dir, "run"), range(5))

    again = _watch(monkeypatch)
    res = tr.main(_argv(first_dir, "--nEpoch", "1", "--restart", "--learningRate", "0.05"))
    assert res.logs["epoch"] == [0] and again["step_count"] == [0] and again["lr"] == [0.05]
    assert res.args.schedulerRamp is None


# ----------------------------------------------------------------------------- 4. a checkpoint the reference wrote
def test_reference_checkpoint_resumes_and_loads(tmp_path, monkeypatch, capsys):
    run_dir = str(tmp_path / "ref_run")
    shutil.copytree(REF_CKPT, run_dir)
    ref = torch.load(os.path.join(run_dir, "checkpoint_7.pt"), "cpu")
    # The fixture's torch.optim.Adam never stepped (its state is empty): a torch.optim.Adam over parameters of the run's shapes,
    # in the run's order (criterion first), takes two steps on seeded gradients and its state goes into the temporary copy.
    assert ref["optimizer"]["state"] == {} and len(ref["optimizer"]["param_groups"][0]["params"]) == 28
    shapes = [tuple(p.shape) for p in tr.loadCriterion(os.path.join(run_dir, "checkpoint_7.pt"), 160, 6).parameters()]
    shapes += [tuple(p.shape) for p in fl.loadModel([os.path.join(run_dir, "checkpoint_7.pt")])[0].parameters()]
    assert len(shapes) == 28
    gen = torch.Generator().manual_seed(21)
    theirs = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    adam = torch.optim.Adam(theirs, lr=2e-4, betas=(0.9, 0.999), eps=1e-8)
    for _ in range(2):
        for p in theirs:
            p.grad = torch.randn(p.shape, generator=gen)
        adam.step()
    ref["optimizer"] = adam.state_dict()
    torch.save(ref, os.path.join(run_dir, "checkpoint_7.pt"))
    with open(os.path.join(run_dir, "checkpoint_logs.json")) as fh:
        assert "saveStep" not in json.load(fh)                     # (somebody's hand-made logs: main fills them)
    seen = _watch(monkeypatch)
    argv = ["--pathDB", DB, "--pathCheckpoint", run_dir, "--path_cache", str(tmp_path / "cache.txt"), "--nGPU", "1",
            "--nEpoch", "2", "--save_step", "1", "--samplingType", "uniform"] + LISTS
    res = tr.main(argv)
    assert res.logs["epoch"] == [7, 1] and res.logs["saveStep"] == 1 and res.args.hiddenEncoder == 32
    assert res.args.samplingType == "samespeaker"                   # the checkpoint's arguments win
    first = seen["first"]
    for name, value in ref["gEncoder"].items():
        assert torch.equal(first["model"][name], value), name
    for name, value in ref["cpcCriterion"].items():
        assert torch.equal(first["criterion"][name], value), name
    ref_step = int(ref["optimizer"]["state"][0]["step"])
    assert ref_step == 2 and seen["step_count"] == [ref_step] and res.optimizer.step_count > ref_step
    for i, st in ref["optimizer"]["state"].items():                # torch.optim.Adam's state, parameter by parameter
        assert torch.equal(first["optimizer"]["state"][i]["exp_avg"].cpu(), st["exp_avg"])
        assert torch.equal(first["optimizer"]["state"][i]["exp_avg_sq"].cpu(), st["exp_avg_sq"])
    assert _finite(res.logs["locLoss_train"][1:]) and _finite(res.logs["locLoss_val"][1:])
    # the new checkpoint loads back
    new = os.path.join(run_dir, "checkpoint_1.pt")
    loaded, _, _ = fl.loadModel([new])
    for name, value in loaded.state_dict().items():
        assert torch.equal(value, res.cpcModel.state_dict()[name].cpu()), name
    torch.optim.Adam([torch.nn.Parameter(torch.zeros_like(p)) for p in res.optimizer.params]).load_state_dict(
        torch.load(new, "cpu")["optimizer"])

    # --load ... --loadCriterion into a fresh directory: epoch 0, the checkpoint's weights in model and criterion
    fresh = str(tmp_path / "fresh")
    started = _watch(monkeypatch)
    res = tr.main(["--pathDB", DB, "--pathCheckpoint", fresh, "--path_cache", str(tmp_path / "cache2.txt"), "--nGPU", "1",
                   "--nEpoch", "1", "--save_step", "1", "--random_seed", "0", "--load", os.path.join(REF_CKPT, "checkpoint_7.pt"),
                   "--loadCriterion"] + LISTS)
    assert res.logs["epoch"] == [0] and started["step_count"] == [0]
    for name, value in ref["gEncoder"].items():
        assert torch.equal(started["first"]["model"][name], value), name
    for name, value in ref["cpcCriterion"].items():
        assert torch.equal(started["first"]["criterion"][name], value), name
    _run_files(fresh, [0])
    assert sorted(os.listdir(REF_CKPT)) == ["checkpoint_7.pt", "checkpoint_args.json", "checkpoint_logs.json"]


# ----------------------------------------------------------------------------- 5. --optimizer sgd
def test_flat_sgd_against_fp64_and_through_main(tmp_path, capsys):
    """cpc_sgd_step: five steps against an fp64 statement of the rule applied to that step's f32 inputs, at the 2e-6 the
    project holds its kernels to against fp64 (tests/test_gpu_parity.py, assert_close)."""
    lib = _lib.load()
    stream = _lib.stream_ptr(torch.device(DEV))
    _lib.check(lib.cpc_async_error_check(stream))                   # (clear anything an earlier test left)
    shapes = [(1024, 1500), (777,), (3, 500, 999)]
    n = sum(int(np.prod(s)) for s in shapes)
    assert n > 3_000_000
    gen = torch.Generator(device="cpu").manual_seed(9)
    params = [torch.nn.Parameter(torch.randn(s, generator=gen).to(DEV)) for s in shapes]
    lr, scale, momentum = 0.03, 0.37, 0.9
    opt = tr.FlatSGD(params, lr=lr)
    assert opt.flat.numel() == n and len(opt.param_groups) == 1
    planted = torch.tensor([12345, n - 7], device=DEV)
    p_start = opt.flat.clone()
    twin = None
    for step in range(1, 6):
        g = torch.randn(n, generator=gen).to(DEV) * (10.0 if step == 4 else 1.0)
        if step != 3:
            g[planted[0]], g[planted[1]] = float("nan"), float("-inf")
        p64, b64, g64 = opt.flat.double(), opt.momentum_buffer.double(), g.double() * scale
        b_ref = g64 if step == 1 else momentum * b64 + g64
        p_ref = p64 - lr * b_ref
        if step != 3:
            b_ref[planted], p_ref[planted] = b64[planted], p64[planted]
        if step == 3:                                               # a state dict taken after two steps, into a fresh optimiser
            sd = opt.state_dict()
            clones = [torch.nn.Parameter(p.detach().clone()) for p in params]
            twin = tr.FlatSGD(clones, lr=lr)
            twin.load_state_dict(sd)
            assert torch.equal(twin.momentum_buffer, opt.momentum_buffer)
            twin.flat_grad.copy_(g)
            twin.step(grad_scale=scale)
        held = (opt.flat[planted].clone(), opt.momentum_buffer[planted].clone())
        opt.flat_grad.copy_(g)
        opt.step(grad_scale=scale)
        if step != 3:                                               # the planted elements: untouched, exactly
            assert torch.equal(opt.flat[planted], held[0]) and torch.equal(opt.momentum_buffer[planted], held[1])
        assert_close(opt.momentum_buffer, b_ref, 2e-6, f"step {step}: momentum buffer")
        assert_close(opt.flat, p_ref, 2e-6, f"step {step}: parameters")
        if step == 3:
            assert torch.equal(twin.flat, opt.flat) and torch.equal(twin.momentum_buffer, opt.momentum_buffer)
            _lib.check(lib.cpc_async_error_check(stream))          # finite gradients: nothing to report
        else:
            with pytest.raises(RuntimeError, match="non-finite gradient"):
                _lib.check(lib.cpc_async_error_check(stream))
            _lib.check(lib.cpc_async_error_check(stream))          # reported once, then clear
        opt.zero_grad()
    assert params[0].data_ptr() == opt.flat.data_ptr() and torch.isfinite(opt.flat).all()
    assert float(opt.momentum_buffer[planted[0]]) != 0.0            # (step 3 moved the planted elements, the others did not)
    assert not torch.equal(opt.flat[planted], p_start[planted])

    # two epochs of main --optimizer sgd, resumed for a third
    run = str(tmp_path / "sgd")
    res = tr.main(_argv(run, "--nEpoch", "2", "--optimizer", "sgd", "--learningRate", "0.01"))
    assert type(res.optimizer) is tr.FlatSGD
    res = tr.main(_argv(run, "--nEpoch", "3"))
    assert type(res.optimizer) is tr.FlatSGD and res.args.optimizer == "sgd" and res.logs["epoch"] == [0, 1, 2]
    logs = _run_files(os.path.join(run, "run"), [0, 1, 2])
    assert _finite(logs["locLoss_train"]) and _finite(logs["locLoss_val"]) and len(logs["locLoss_train"]) == 3
    state = torch.load(os.path.join(run, "run", "checkpoint_2.pt"), "cpu")["optimizer"]
    theirs = [torch.nn.Parameter(torch.zeros(p.shape)) for p in res.optimizer.params]
    ref = torch.optim.SGD(theirs, lr=1.0, momentum=0.9)
    ref.load_state_dict(state)
    assert ref.param_groups[0]["lr"] == 0.01 and ref.param_groups[0]["momentum"] == 0.9
    assert all(ref.state[p]["momentum_buffer"].shape == p.shape for p in theirs)
    assert any(float(ref.state[p]["momentum_buffer"].abs().sum()) > 0 for p in theirs)


# ----------------------------------------------------------------------------- 6. --no_artefacts
@pytest.mark.parametrize("extra,sampling,batch,convention", [
    (["--no_artefacts", "--samplingType", "samespeaker"], "samespeaker", 8, None),
    (["--samplingType", "temporalsamespeaker", "--naming_convention", "spkr-id", "--no_artefacts", "--batchSizeGPU", "2"],
     "temporalsamespeaker", 2, "spkr-id"),
], ids=["samespeaker", "temporalsamespeaker"])
def test_no_artefacts_runs_and_device_loader_follows_the_cpu_loader(extra, sampling, batch, convention, tmp_path, capsys):
    res = tr.main(_argv(str(tmp_path), "--nEpoch", "2", *extra, lists=convention is None))
    assert res.args.no_artefacts and res.logs["epoch"] == [0, 1]
    for key in ("locLoss_train", "locLoss_val"):
        assert len(res.logs[key]) == 2 and _finite(res.logs[key]), key
    seqs, speakers = ds.findAllSeqs(DB, extension=".flac", format=convention)
    seqs = sorted(seqs, key=lambda s: s[1]) if convention is None else seqs
    yielded = {}
    for device in ("cpu", DEV):
        random.seed(4)
        torch.manual_seed(4)
        data = ds.AudioBatchData(DB, 20480, seqs, None, len(speakers), keep_temporality=sampling == "temporalsamespeaker",
                                 device=device)
        loader = data.getDataLoader(batch, sampling, True, remove_artefacts=True, batch_size_per_gpu=batch)
        yielded[device] = [(x.cpu().clone(), y.cpu().clone()) for x, y in loader]
        bounds = data.seqLabel
    assert len(yielded["cpu"]) == len(yielded[DEV]) > 0
    for (xc, yc), (xg, yg) in zip(yielded["cpu"], yielded[DEV]):
        assert torch.equal(xc, xg) and torch.equal(yc, yg)         # the same windows: they start where the CPU loader's do
    assert len(bounds) == 10


# ----------------------------------------------------------------------------- 7. the module entry point
def _child(argv, extra_env=None):
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.update(extra_env or {})
    return subprocess.run([sys.executable, "-m", "cpc2_amd.train"] + argv, cwd=ROOT, env=env, timeout=300,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_module_entry_point_as_a_child_process(tmp_path):
    plain = _child(_argv(str(tmp_path / "plain"), "--nEpoch", "2"))
    assert plain.returncode == 0, plain.stdout[-3000:]
    assert "CONFIG:" in plain.stdout and "Running 2 epochs" in plain.stdout
    logs = _run_files(str(tmp_path / "plain" / "run"), [0, 1])
    assert logs["epoch"] == [0, 1] and _finite(logs["locLoss_train"])

    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = str(s.getsockname()[1])
    s.close()
    world = {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": port}
    dist = _child(_argv(str(tmp_path / "dist"), "--nEpoch", "2", "--distributed"), world)
    assert dist.returncode == 0, dist.stdout[-3000:]
    logs_dist = _run_files(str(tmp_path / "dist" / "run"), [0, 1])
    assert logs_dist["epoch"] == [0, 1] and _finite(logs_dist["locLoss_train"])
    assert sorted(os.listdir(tmp_path / "dist" / "run")) == sorted(os.listdir(tmp_path / "plain" / "run"))
    with open(tmp_path / "dist" / "run" / "checkpoint_args.json") as fh:
        written = json.load(fh)
    assert written["distributed"] is True and written["is_local_master"] is True and written["global_rank"] == 0
