"""Whole-utterance phone recognition without a GPU (cpc2_amd/eval/common_voices_eval.py against tests/golden/g27_common_voice.npz,
tools/make_golden_common_voice.py): the two sub-commands parse to the reference's defaults, every deviation that is a refusal is
raised by name before the data set is listed, CTCphone_criterion has the reference's state dict and seeded init, the dataset's
bookkeeping and cut_data equal the reference's, the fp64 oracle (tests/ctc_head_oracle.py) reproduces the recorded getPrediction
and agrees with torch's own CTC in float64, checkpoints load with and without the `module.` prefix, and the library declares the
new entry points and refuses sizes outside its limits with a message."""
import ctypes
import json
import os
import random
import re

import numpy as np
import pytest
import torch

import ctc_head_oracle as oracle
from cpc2_amd import _lib
from cpc2_amd.dataset import findAllSeqs, parseSeqLabels
from cpc2_amd.eval import common_voices_eval as cv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DB = os.path.join(GOLDEN, "test_db")
TRANSCRIPTS = os.path.join(GOLDEN, "g27_phone_transcripts.txt")
MISSING = os.path.join(GOLDEN, "no_such_directory")
NEW = ("cpc_ctc_loss_scratch_bytes", "cpc_ctc_loss", "cpc_seqnorm_len_forward", "cpc_seqnorm_len_backward",
       "cpc_conv_head_forward_scratch_bytes", "cpc_conv_head_forward", "cpc_conv_head_backward_data", "cpc_gather_utterances")


# ----------------------------------------------------------------------------- command line
def test_train_flags_parse_to_the_reference_defaults():
    args = vars(cv.parse_args(["train", "DB", "PHONE", "CKPT"]))
    assert args == dict(command="train", pathDB="DB", pathPhone="PHONE", pathCheckpoint="CKPT", freeze=False, pathTrain=None,
                        pathVal=None, file_extension=".wav", batchSize=8, nEpochs=30, beta1=0.9, beta2=0.999, epsilon=1e-08,
                        lr=2e-04, output="out", debug=False, no_pretraining=False, LSTM=False, seqNorm=False, kernelSize=8,
                        dropout=False, in_dim=1, loss_reduction="mean", roffset=0, augments=None, t_ms=100)
    args = cv.parse_args(["train", "DB", "PHONE", "CKPT", "--freeze", "--pathTrain", "T", "--pathVal", "V", "--file_extension", ".flac",
                          "--batchSize", "4", "--nEpochs", "2", "--beta1", "0.8", "--beta2", "0.9", "--epsilon", "1e-6", "--lr", "1e-3",
                          "-o", "O", "--debug", "--no_pretraining", "--LSTM", "--seqNorm", "--kernelSize", "4", "--dropout",
                          "--in_dim", "2", "--loss_reduction", "sum", "--roffset", "80", "-a", '{"a": 1}', "--t_ms", "50"])
    assert (args.freeze, args.pathTrain, args.pathVal, args.file_extension, args.batchSize, args.nEpochs) == (True, "T", "V", ".flac", 4, 2)
    assert (args.beta1, args.beta2, args.epsilon, args.lr, args.output, args.debug) == (0.8, 0.9, 1e-6, 1e-3, "O", True)
    assert (args.no_pretraining, args.LSTM, args.seqNorm, args.kernelSize, args.dropout, args.in_dim) == (True, True, True, 4, True, 2)
    assert (args.loss_reduction, args.roffset, args.augments, args.t_ms) == ("sum", 80, [{"a": 1}], 50)


def test_per_flags_parse_to_the_reference_defaults():
    assert vars(cv.parse_args(["per", "OUT"])) == dict(command="per", output="OUT", batchSize=8, debug=False, pathDB=None,
                                                       pathVal=None, pathPhone=None, file_extension=".wav", name="0")
    args = cv.parse_args(["per", "OUT", "--batchSize", "2", "--debug", "--pathDB", "D", "--pathVal", "V", "--pathPhone", "P",
                          "--file_extension", ".flac", "--name", "t"])
    assert (args.batchSize, args.debug, args.pathDB, args.pathVal, args.pathPhone, args.file_extension, args.name) == (
        2, True, "D", "V", "P", ".flac", "t")


REFUSED = [(["--file_extension", ".mp3"], "CKPT", r"--file_extension \.mp3"),
           ([], "ID", r"pathCheckpoint ID"),
           (["--in_dim", "2"], "CKPT", r"--in_dim 2"),
           (["--augments", '{"type": "pitch"}'], "CKPT", r"--augments"),
           (["--kernelSize", "4"], "CKPT", r"--kernelSize 4")]


@pytest.mark.parametrize("flags,checkpoint,word", REFUSED, ids=[r[2] for r in REFUSED])
def test_train_refuses_by_name_before_the_data_set_is_listed(flags, checkpoint, word, monkeypatch, tmp_path):
    listed = []
    monkeypatch.setattr(cv, "findAllSeqs", lambda *a, **k: listed.append(a) or ([], []))
    out = tmp_path / "out"
    with pytest.raises(ValueError, match=word):
        cv.main(["train", MISSING, TRANSCRIPTS, checkpoint, "-o", str(out)] + flags)
    assert not listed and not out.exists() and not os.path.exists(MISSING)


def test_per_refuses_an_mp3_run_before_the_data_set_is_listed(monkeypatch, tmp_path):
    listed = []
    monkeypatch.setattr(cv, "findAllSeqs", lambda *a, **k: listed.append(a) or ([], []))
    with open(tmp_path / "args_training.json", "w") as f:
        json.dump(dict(pathDB=MISSING, file_extension=".mp3", pathPhone=TRANSCRIPTS, pathVal=None, pathCheckpoint="CKPT",
                       no_pretraining=False), f)
    with pytest.raises(ValueError, match=r"--file_extension \.mp3"):
        cv.main(["per", str(tmp_path)])
    with open(tmp_path / "args_training.json", "w") as f:
        json.dump(dict(pathDB=MISSING, file_extension=".flac", pathPhone=TRANSCRIPTS, pathVal=None, pathCheckpoint="ID",
                       no_pretraining=False, in_dim=1), f)
    with pytest.raises(ValueError, match=r"pathCheckpoint ID"):
        cv.main(["per", str(tmp_path)])
    assert not listed and not (tmp_path / "logs_per_0.txt").exists()


def test_get_per_args_reads_the_training_run(tmp_path):
    with open(tmp_path / "args_training.json", "w") as f:
        json.dump(dict(pathDB="D", file_extension=".flac", pathPhone="P", pathVal="V", pathCheckpoint="C", no_pretraining=True,
                       LSTM=True, seqNorm=True), f)
    args = cv.get_PER_args(cv.parse_args(["per", str(tmp_path)]))
    assert (args.pathDB, args.file_extension, args.pathPhone, args.pathVal, args.pathCheckpoint) == ("D", ".flac", "P", "V", "C")
    assert (args.no_pretraining, args.LSTM, args.seqNorm, args.dropout, args.in_dim, args.loss_reduction) == (
        True, True, True, False, 1, "mean")
    args = cv.get_PER_args(cv.parse_args(["per", str(tmp_path), "--pathDB", "D2", "--pathVal", "V2"]))
    assert (args.pathDB, args.file_extension, args.pathVal, args.pathPhone) == ("D2", ".wav", "V2", None)


# ----------------------------------------------------------------------------- the criterion's parameters
def test_state_dict_and_seeded_init_equal_the_reference(golden):
    g = golden("g27_common_voice.npz")
    torch.manual_seed(27)
    crit = cv.CTCphone_criterion(32, 5)
    state = crit.state_dict()
    assert list(state.keys()) == json.loads(str(g["sd_keys"]))
    assert set(state.keys()) == {"PhoneCriterionClassifier.weight", "PhoneCriterionClassifier.bias", "conv1.weight_ih_l0",
                                 "conv1.weight_hh_l0", "conv1.bias_ih_l0", "conv1.bias_hh_l0"}
    for k, v in state.items():
        assert list(v.shape) == list(g[f"sd_{k}_shape"])
        assert v.double().abs().sum().item() == pytest.approx(float(g[f"sd_{k}_abssum"]), rel=1e-12)
    assert crit.BLANK_LABEL == 5 and crit.downsampling_factor == 4 and crit.epsilon == 1e-8 and crit.dropout is None
    assert isinstance(cv.CTCphone_criterion(32, 5, dropout=True).dropout, torch.nn.Dropout)
    with pytest.raises(ValueError, match="sizeKernel=7"):
        cv.CTCphone_criterion(32, 5, sizeKernel=7)


def test_checkpoints_load_with_and_without_the_module_prefix():
    torch.manual_seed(1)
    src = cv.CTCphone_criterion(8, 3)
    model = torch.nn.Linear(4, 4)
    plain = dict(classifier=src.state_dict(), model=model.state_dict())
    prefixed = dict(classifier=cv._with_prefix(src.state_dict()), model=cv._with_prefix(model.state_dict()), bestLoss=1.0)
    assert all(k.startswith("module.") for k in prefixed["classifier"]) and all(k.startswith("module.") for k in prefixed["model"])
    for state in (plain, prefixed):
        torch.manual_seed(2)
        crit, other = cv.CTCphone_criterion(8, 3), torch.nn.Linear(4, 4)
        cv.load_checkpoint(state, other, crit)
        for k, v in src.state_dict().items():
            assert torch.equal(crit.state_dict()[k], v)
        assert torch.equal(other.weight, model.weight)


# ----------------------------------------------------------------------------- the dataset
@pytest.fixture(scope="module")
def nine():
    seqs, _ = findAllSeqs(DB, extension=".flac")
    labels, n_phones = parseSeqLabels(TRANSCRIPTS)
    assert len(seqs) == 9 and n_phones == 41
    return seqs, labels


@pytest.mark.parametrize("amp", [0, 80])
def test_dataset_bookkeeping_and_items_equal_the_reference(golden, nine, amp):
    g = golden("g27_common_voice.npz")
    seqs, labels = nine
    ds = cv.SingleSequenceDataset(DB, seqs, labels, random_offset_amplitude=amp, device="cpu")
    assert ds.seqOffset == g["ds_seqOffset"].tolist() and ds.phoneOffsets == g["ds_phoneOffsets"].tolist()
    assert (ds.maxSize, ds.maxSizePhone, len(ds)) == (int(g["ds_maxSize"]), int(g["ds_maxSizePhone"]), int(g["ds_len"])) and len(ds) == 9
    random.seed(27)
    for idx in range(len(ds)):
        seq, size_seq, phone, size_phone = ds[idx]
        assert seq.shape == (1, ds.maxSize) and seq.dtype == torch.float32
        assert size_seq.dtype == phone.dtype == size_phone.dtype == torch.long and size_seq.shape == size_phone.shape == (1,)
        n = int(size_seq)
        assert n == g[f"ds{amp}_sizeSeq"][idx] and int(size_phone) == g[f"ds{amp}_sizePhone"][idx]
        assert np.array_equal(phone.numpy(), g[f"ds{amp}_phone"][idx])
        assert seq.double().sum().item() == pytest.approx(float(g[f"ds{amp}_sum"][idx]), rel=1e-12, abs=1e-12)
        assert np.array_equal(seq[0, :8].numpy(), g[f"ds{amp}_head"][idx])
        edge = seq[0, n - 4:n + 4].numpy()
        assert np.array_equal(edge, g[f"ds{amp}_edge"][idx][:len(edge)])
    if amp:
        full = np.diff(g["ds_seqOffset"])
        assert (g["ds80_sizeSeq"] <= full).all() and (g["ds80_sizeSeq"] >= full - 80).all() and (g["ds80_sizeSeq"] != full).any()


def test_dataset_refuses_what_the_port_does_not_read(nine):
    seqs, labels = nine
    with pytest.raises(ValueError, match="inDim=2"):
        cv.SingleSequenceDataset(MISSING, seqs, labels, inDim=2, device="cpu")
    with pytest.raises(ValueError, match="transform"):
        cv.SingleSequenceDataset(MISSING, seqs, labels, transform=lambda x: x, device="cpu")


def test_cut_data_equals_the_reference(golden):
    g = golden("g27_common_voice.npz")
    out = cv.cut_data(torch.from_numpy(g["cut_in"]), torch.from_numpy(g["cut_sizes"]))
    assert np.array_equal(out.numpy(), g["cut_out"]) and out.shape == (4, 7, 3)


# ----------------------------------------------------------------------------- the oracle
def _case(g, i):
    state = {k[len(f"gp{i}_p_"):]: g[k] for k in g.files if k.startswith(f"gp{i}_p_")}
    seq_norm, lstm = (bool(v) for v in g[f"gp{i}_flags"])
    return g[f"gp{i}_c"], g[f"gp{i}_sizes"], state, seq_norm, lstm, g[f"gp{i}_pred"]


def test_golden_holds_the_cases_of_the_issue(golden):
    g = golden("g27_common_voice.npz")
    assert sorted(tuple(g[f"gp{i}_flags"]) for i in range(4)) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    for i in range(4):
        c, sizes, state, _, _, pred = _case(g, i)
        assert c.shape == (3, 40, 32) and c.dtype == np.float64 and sizes.tolist() == [40, 33, 21] and pred.shape == (3, 9, 6)
        assert state["PhoneCriterionClassifier.weight"].shape == (6, 32, 8)


@pytest.mark.parametrize("i", range(4))
def test_oracle_reproduces_the_recorded_predictions(golden, i):
    c, sizes, state, seq_norm, lstm, pred = _case(golden("g27_common_voice.npz"), i)
    mine = oracle.criterion(c, sizes, state, seq_norm, lstm)["pred"]
    assert np.abs(mine - pred).max() <= 1e-12 * max(1.0, np.abs(pred).max())


def test_oracle_pieces_agree_with_each_other(golden):
    """The numpy seqNorm and classifier equal the torch statement inside oracle.criterion, and their closed-form gradients equal
    torch.autograd's, in float64."""
    c, sizes, state, _, _, _ = _case(golden("g27_common_voice.npz"), 0)
    w, b = state["PhoneCriterionClassifier.weight"], state["PhoneCriterionClassifier.bias"]
    y = oracle.seqnorm_len(c, sizes)
    pred = oracle.criterion(c, sizes, state, True, False)["pred"]
    assert np.abs(oracle.conv_head(y, w, b) - pred).max() < 1e-12
    rng = np.random.default_rng(3)
    for s in (40, 43):
        x = rng.standard_normal((3, s, 32))
        xt = torch.tensor(x, requires_grad=True)
        wt, bt = torch.tensor(w, requires_grad=True), torch.tensor(b, requires_grad=True)
        out = torch.nn.functional.conv1d(xt.permute(0, 2, 1), wt, bt, stride=4).permute(0, 2, 1)
        dout = rng.standard_normal(tuple(out.shape))
        out.backward(torch.tensor(dout))
        dw, db, dx = oracle.conv_head_backward(x, w, dout)
        assert np.abs(oracle.conv_head(x, w, b) - out.detach().numpy()).max() < 1e-12
        assert np.abs(dw - wt.grad.numpy()).max() < 1e-11 and np.abs(db - bt.grad.numpy()).max() < 1e-11
        assert np.abs(dx - xt.grad.numpy()).max() < 1e-12
        assert (dx[:, 4 * (out.shape[1] + 1):] == 0).all()


def _ctc_case(pred, seed):
    rng = np.random.default_rng(seed)
    b, t, k = pred.shape
    in_len = np.array([t, t - 2, 5][:b])
    tgt_len = np.array([4, 3, 2][:b])
    targets = rng.integers(0, k - 1, (b, 6))
    targets[0, 1] = targets[0, 0]                       # a repeated label
    return in_len, targets, tgt_len


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("i", range(4))
def test_oracle_ctc_agrees_with_torch_in_float64(golden, i, reduction):
    pred = _case(golden("g27_common_voice.npz"), i)[5]
    in_len, targets, tgt_len = _ctc_case(pred, 10 + i)
    loss, nll, grad = oracle.ctc_len(pred, in_len, targets, tgt_len, reduction)
    logits = torch.tensor(pred, requires_grad=True)
    ref = torch.nn.functional.ctc_loss(torch.log_softmax(logits, 2).permute(1, 0, 2), torch.tensor(targets), torch.tensor(in_len),
                                       torch.tensor(tgt_len), blank=pred.shape[2] - 1, reduction=reduction, zero_infinity=True)
    ref.backward()
    assert abs(loss - ref.item()) <= 1e-10 * max(1.0, abs(ref.item()))
    assert np.abs(grad - logits.grad.numpy()).max() <= 1e-10
    for row, n in enumerate(in_len):
        assert (grad[row, n:] == 0).all() and np.abs(grad[row, :n]).max() > 0


@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_oracle_ctc_agrees_with_torch_in_float64_past_256_states(reduction):
    """The same comparison on the rows of oracle.ctc_long_case (128 to 150 labels: 257 to 301 extended states), which the GPU
    tests hold ctc_len_kernel to where a thread owns more than one state.  The gradient row by row against that row's largest
    element: under the mean reduction the empty transcription's row is a hundred times the long rows'."""
    logits, in_len, targets, tgt_len = oracle.ctc_long_case()
    assert logits.shape == (9, 300, 41) and (2 * tgt_len[:8] + 1 > 256).all() and tgt_len[8] == 0
    assert (targets[2, 126:130] == targets[2, 126]).all() and (np.diff(targets[3]) != 0).all() and (targets[6] == 3).all()
    loss, nll, grad = oracle.ctc_len(logits, in_len, targets, tgt_len, reduction)
    for row in range(9):                                # rows 5 and 7 are one frame short of an alignment
        assert (nll[row] == 0) == (row in oracle.CTC_LONG_INFEASIBLE) and nll[row] >= 0
    x = torch.tensor(logits.astype(np.float64), requires_grad=True)
    ref = torch.nn.functional.ctc_loss(torch.log_softmax(x, 2).permute(1, 0, 2), torch.tensor(targets), torch.tensor(in_len),
                                       torch.tensor(tgt_len), blank=40, reduction=reduction, zero_infinity=True)
    ref.backward()
    ref_grad = x.grad.numpy()
    assert abs(loss - ref.item()) <= 1e-10 * max(1.0, abs(ref.item()))
    for row, n in enumerate(in_len):
        if row in oracle.CTC_LONG_INFEASIBLE:
            assert (grad[row] == 0).all() and (ref_grad[row] == 0).all()
            continue
        assert np.abs(grad[row] - ref_grad[row]).max() <= 1e-10 * np.abs(ref_grad[row]).max()
        assert (grad[row, n:] == 0).all() and np.abs(grad[row, :n]).max() > 0


def test_oracle_ctc_edge_cases():
    rng = np.random.default_rng(5)
    logits = rng.standard_normal((3, 7, 4))
    targets = np.array([[0, 0, 1], [2, 1, 0], [1, 1, 1]])
    # row 0: "0 0 1" needs 4 frames and has 3 (no alignment); row 1: an input length of 0; row 2: an empty transcription
    loss, nll, grad = oracle.ctc_len(logits, [3, 0, 7], targets, [3, 2, 0], "sum")
    assert nll[0] == 0 and nll[1] == 0 and (grad[:2] == 0).all()
    lp = logits[2] - np.log(np.exp(logits[2]).sum(axis=1, keepdims=True))
    assert nll[2] == pytest.approx(-lp[:, 3].sum(), rel=1e-12) and loss == pytest.approx(nll[2], rel=1e-12)


# ----------------------------------------------------------------------------- the library's interface
def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "cpc2_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in cpc2_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES
    assert _lib.load().cpc_version() >= 117


def test_ctc_loss_scratch_query_returns_zero_with_a_message_outside_the_limits():
    lib = _lib.load()
    query = lib.cpc_ctc_loss_scratch_bytes
    # f64 [b][t_max] and [b][t_max][2 max_l + 1], f64 [b] and int [b], each rounded up to 256 bytes
    assert query(6, 37, 9) == 256 * -(-(8 * 6 * 37) // 256) + 256 * -(-(8 * 6 * 37 * 19) // 256) + 256 + 256
    assert query(1, 4096, 1024) > 0 and query(1, 1, 0) > 0
    for bad, word in [((0, 37, 9), b"b=0"), ((65536, 37, 9), b"b=65536"), ((6, 0, 0), b"t_max=0"), ((6, 4097, 9), b"t_max=4097"), ((6, 37, 38), b"max_l=38"),
                      ((6, 37, -1), b"max_l=-1"), ((1, 4096, 1025), b"max_l=1025")]:
        assert query(*bad) == 0
        message = lib.cpc_last_error()
        assert message.startswith(b"ctc_loss:") and word in message, message


def test_entries_refuse_by_name_before_any_gpu_call():
    """Every call is refused on its sizes, and every pointer is NULL: whatever order an entry checks in, nothing is launched."""
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    assert lib.cpc_ctc_loss(null, 6, 37, 1, null, null, 9, null, 1, null, null, null, null, 0, null) == -1
    assert b"ctc_loss:" in lib.cpc_last_error() and b"k=1" in lib.cpc_last_error()
    assert lib.cpc_ctc_loss(null, 6, 37, 6, null, null, 9, null, 2, null, null, null, null, 0, null) == -1
    assert b"ctc_loss: reduction 2" in lib.cpc_last_error()
    assert lib.cpc_seqnorm_len_forward(null, null, 0, 40, 32, 1e-8, null, null, null, null) == -1
    assert b"seqnorm_len_forward:" in lib.cpc_last_error()
    assert lib.cpc_seqnorm_len_backward(null, null, null, null, 3, 0, 32, null, null) == -1
    assert b"seqnorm_len_backward:" in lib.cpc_last_error()
    assert lib.cpc_conv_head_backward_data(null, null, 3, 40, 32, 6, 7, null, null) == -1
    assert b"conv_head_backward_data: kernel size 7" in lib.cpc_last_error()
    assert lib.cpc_conv_head_backward_data(null, null, 3, 7, 32, 6, 8, null, null) == -1
    assert b"conv_head_backward_data:" in lib.cpc_last_error() and b"s=7" in lib.cpc_last_error()
    assert lib.cpc_conv_head_forward_scratch_bytes(3, 40, 32, 6, 8) > 0 and lib.cpc_conv_head_forward_scratch_bytes(8, 1500, 256, 42, 8) > 256
    assert lib.cpc_conv_head_forward_scratch_bytes(3, 7, 32, 6, 8) == 0
    assert b"conv_head_forward:" in lib.cpc_last_error() and b"s=7" in lib.cpc_last_error()
    assert lib.cpc_conv_head_forward(null, null, null, null, 3, 40, 32, 6, 6 + 1, null, 0, null) == -1
    assert b"conv_head_forward: kernel size 7" in lib.cpc_last_error()
    assert lib.cpc_gather_utterances(null, 10, null, null, null, null, 0, 5, null) == -1
    assert b"gather_utterances:" in lib.cpc_last_error()


def test_probe_ctc_shares_the_scratch_and_the_batch_limit_of_ctc_loss():
    """cpc_probe_ctc runs on cpc_ctc_loss's kernels (version 122): the same room inside the probe's own limits, 0 outside them,
    and b <= 65535.  Every pointer is NULL: nothing is launched."""
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    assert lib.cpc_version() >= 122
    for b, t, max_l in [(1, 1, 0), (8, 128, 128), (3, 1024, 1024)]:
        assert lib.cpc_probe_ctc_scratch_bytes(b, t, max_l) == lib.cpc_ctc_loss_scratch_bytes(b, t, max_l) > 0
    for b, t, max_l in [(8, 1025, 128), (8, 128, 129), (0, 128, 128)]:
        assert lib.cpc_probe_ctc_scratch_bytes(b, t, max_l) == 0
    assert lib.cpc_probe_ctc(null, 65536, 37, 6, null, 9, null, null, null, null, null, 0, null) == -1
    message = lib.cpc_last_error()
    assert message.startswith(b"probe_ctc: sizes outside the supported limits") and b"b=65536" in message, message
    # in_lengths is optional inside the library only: the public entry still refuses a call without it.  Sizes in range and the
    # other required pointers non-NULL (never dereferenced); without scratch the call could not reach a launch in any case
    some = ctypes.c_void_p(256)
    assert lib.cpc_ctc_loss(some, 6, 37, 6, null, some, 9, some, 1, some, some, null, null, 0, null) == -1
    assert lib.cpc_last_error() == b"ctc_loss: null buffer"


def test_ctc_loss_and_conv_head_refuse_every_size_outside_their_limits_before_any_gpu_call():
    """The limits the GPU tests run AT (4096 frames, 1024 labels, max_l = t_max, 2 classes; even kernel sizes from 2 and
    s = ks), each passed by one.  Every pointer is NULL, as above."""
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    for (b, t, k, max_l), word in [((6, 4097, 6, 9), b"t_max=4097"), ((1, 4096, 6, 1025), b"max_l=1025"), ((6, 37, 6, 38), b"max_l=38"),
                                   ((65536, 37, 6, 9), b"b=65536"), ((6, 37, 1, 9), b"k=1"), ((6, 37, 0, 9), b"k=0"),
                                   ((6, 37, 65537, 9), b"k=65537")]:
        assert lib.cpc_ctc_loss(null, b, t, k, null, null, max_l, null, 1, null, null, null, null, 0, null) == -1
        message = lib.cpc_last_error()
        assert message.startswith(b"ctc_loss: sizes outside the supported limits") and word in message, message
    for s, ks, word in [(40, 3, b"kernel size 3"), (40, 0, b"kernel size 0"), (40, -2, b"kernel size -2"), (1, 2, b"s=1"),
                        (15, 16, b"s=15")]:
        assert lib.cpc_conv_head_forward_scratch_bytes(3, s, 32, 6, ks) == 0
        message = lib.cpc_last_error()
        assert message.startswith(b"conv_head_forward:") and word in message, message
        assert lib.cpc_conv_head_forward(null, null, null, null, 3, s, 32, 6, ks, null, 0, null) == -1
        message = lib.cpc_last_error()
        assert message.startswith(b"conv_head_forward:") and word in message, message
        assert lib.cpc_conv_head_backward_data(null, null, 3, s, 32, 6, ks, null, null) == -1
        message = lib.cpc_last_error()
        assert message.startswith(b"conv_head_backward_data:") and word in message, message
    assert lib.cpc_conv_head_forward_scratch_bytes(3, 2, 32, 6, 2) > 0 and lib.cpc_conv_head_forward_scratch_bytes(3, 16, 32, 6, 16) > 0
