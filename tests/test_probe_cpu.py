"""Linear-separability probe without a GPU: the fp64 oracle against torch's float64 CTC, the phone labels of the feeder
(parseSeqLabels, window labels on device="cpu") and collapseLabelChain's expectations against golden g21 (recorded from the
reference by tools/make_golden_probe.py), the command line's defaults and refusals, and the reference's log arithmetic."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

import probe_oracle as PO
from cpc2_amd.dataset import AudioBatchData, findAllSeqs, parseSeqLabels
from cpc2_amd.eval import linear_separability as LS
from cpc2_amd.train import update_logs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DB = os.path.join(GOLDEN, "test_db")
PHONES = os.path.join(GOLDEN, "phone_labels.txt")


@pytest.fixture(scope="module")
def g21():
    z = np.load(os.path.join(GOLDEN, "g21_linear_separability.npz"), allow_pickle=False)
    return z, json.loads(str(z["meta"]))


def _torch_ctc(logits, targets, lengths):
    B, T, K = logits.shape
    flat = torch.cat([torch.from_numpy(np.asarray(targets[i][:lengths[i]], np.int64)) for i in range(B)])
    x = torch.from_numpy(logits).double().requires_grad_(True)
    loss = torch.nn.functional.ctc_loss(torch.log_softmax(x, 2).permute(1, 0, 2), flat, torch.full((B,), T, dtype=torch.long),
                                        torch.tensor(lengths, dtype=torch.long), blank=K - 1, reduction="mean",
                                        zero_infinity=True)
    loss.backward()
    return loss.item(), x.grad.numpy()


@pytest.mark.parametrize("case", ["typical", "empty_and_infeasible", "repeats", "wide"])
def test_ctc_oracle_matches_torch_float64(case):
    rng = np.random.default_rng(["typical", "empty_and_infeasible", "repeats", "wide"].index(case) + 7)
    T, K = (40, 7) if case != "wide" else (24, 70)
    B = 5
    logits = rng.standard_normal((B, T, K)) * 2
    if case == "typical":
        lengths = [5, 12, 1, 8, 20]
        targets = [rng.integers(0, K - 1, size=L) for L in lengths]
    elif case == "empty_and_infeasible":
        lengths = [0, 3, 30, 0, 10]
        targets = [rng.integers(0, K - 1, size=L) for L in lengths]
        targets[2] = np.zeros(30, np.int64)               # 30 equal labels need 59 frames > 40: infeasible
    elif case == "repeats":
        lengths = [6, 6, 10, 4, 2]
        targets = [np.array([1, 1, 2, 2, 2, 3]), np.array([0, 0, 0, 0, 0, 0]), rng.integers(0, 2, size=10),
                   np.array([5, 5, 5, 5]), np.array([3, 3])]
    else:
        lengths = [10, 0, 23, 5, 12]
        targets = [rng.integers(0, K - 1, size=L) for L in lengths]
    loss, nll, grad = PO.ctc(logits, targets, lengths)
    tloss, tgrad = _torch_ctc(logits, targets, lengths)
    assert abs(loss - tloss) <= 1e-10 * max(1.0, abs(tloss))
    assert np.abs(grad - tgrad).max() <= 1e-10
    if case == "empty_and_infeasible":
        assert nll[2] == 0.0 and np.all(grad[2] == 0.0)
        # an empty target: -sum log p(blank)
        lp = logits[0] - np.log(np.exp(logits[0]).sum(axis=1, keepdims=True))
        assert abs(nll[0] + lp[:, K - 1].sum()) <= 1e-9


def test_xent_oracle_matches_torch_float64():
    rng = np.random.default_rng(3)
    x, w, b = rng.standard_normal((37, 19)), rng.standard_normal((11, 19)), rng.standard_normal(11)
    y = rng.integers(0, 11, size=37)
    o = PO.xent(x, w, b, y)
    xt, wt, bt = (torch.from_numpy(a).requires_grad_(True) for a in (x, w, b))
    z = torch.nn.functional.linear(xt, wt, bt)
    loss = torch.nn.functional.cross_entropy(z, torch.from_numpy(y))
    loss.backward()
    assert abs(o["loss"] - loss.item()) < 1e-12
    for name, t in (("dX", xt), ("dW", wt), ("db", bt)):
        assert np.abs(o[name] - t.grad.numpy()).max() < 1e-12
    assert o["acc"] == float((z.max(1)[1] == torch.from_numpy(y)).double().mean())


def test_parse_seq_labels(g21):
    z, meta = g21
    labels, n_phones = parseSeqLabels(PHONES)
    assert n_phones == meta["n_phones"] == 41
    assert labels["step"] == meta["step"] == 160
    assert len(labels) - 1 == meta["n_label_lines"]
    for name in ("2911-12359-0007", "4051-11218-0044"):
        assert labels[name] == z[f"labels_{name}"].tolist()


def _labelled_dataset(meta):
    labels, _ = parseSeqLabels(PHONES)
    seqs = [tuple(s) for s in meta["seqs"]]
    return AudioBatchData(DB, 20480, seqs, labels, meta["n_speakers"], device="cpu")


def test_window_labels_match_reference(g21):
    z, meta = g21
    db = _labelled_dataset(meta)
    assert db.phoneSize == 160 and db.phoneStep == 128 and not db.doubleLabels
    assert db.data.numel() == meta["data_size"]            # each file cut to len(labels) * 160 samples
    assert db.seqLabel == meta["seq_label"] and db.speakerLabel == meta["speaker_label"]
    for o, expect in zip(z["offsets"].tolist(), z["phonem"]):
        assert db.getPhonem(o) == expect.tolist()
    # the device gather (here on the CPU) gives the same rows
    got = db.phonemes_from(torch.tensor(z["offsets"]))
    assert np.array_equal(got.numpy(), z["phonem"])
    # the sequential loader yields the phone labels in place of the speaker's
    batches = db.getBaseSampler("sequential", 2, 0)
    got = [lab for _x, lab in db.getDataLoader(2, "sequential", False)]
    assert len(got) == len(batches) >= 2
    for lab, offs in zip(got, batches):
        assert lab.dtype == torch.long and lab.tolist() == [db.getPhonem(o) for o in offs]


def test_missing_labels_raise_key_error(g21):
    _z, meta = g21
    labels, _ = parseSeqLabels(PHONES)
    seqs, speakers = findAllSeqs(DB, extension=".flac")
    unlabelled = [s for s in seqs if "5393-19218-0024" in s[1]]
    with pytest.raises(KeyError):
        AudioBatchData(DB, 20480, unlabelled, labels, len(speakers), device="cpu")


def test_collapse_oracle_matches_reference(g21):
    z, _ = g21
    for tag, rows in (("all", slice(None)), ("three", slice(2, 5)), ("one", slice(7, 8))):
        out, sizes = PO.collapse(z["phonem"][rows])
        assert np.array_equal(out, z[f"collapse_{tag}_out"]) and np.array_equal(sizes, z[f"collapse_{tag}_sizes"])


def test_parse_args_defaults_and_save_step(g21):
    _z, meta = g21
    a = vars(LS.parse_args(["db", "train.txt", "val.txt", "ckpt.pt"]))
    ref = meta["parse_args_defaults"]
    assert a["nGPU"] == 1
    for key, value in ref.items():
        if key in ("load", "pathCheckpoint"):
            continue
        assert a[key] == value, key
    assert a["save_step"] == a["n_epoch"] == 10
    assert LS.parse_args(["d", "t", "v", "c", "--save_step", "0", "--n_epoch", "3"]).save_step == 3
    assert LS.parse_args(["d", "t", "v", "c", "--save_step", "2"]).save_step == 2
    assert LS.parse_args(["d", "t", "v", "c", "--ignore_cache"]).ignore_cache


@pytest.mark.parametrize("argv,kind", [
    (["--CTC", "--get_encoded", "--pathPhone", PHONES], ValueError),
    (["--nGPU", "2"], SystemExit),
])
def test_refusals(argv, kind, tmp_path):
    with pytest.raises(kind):
        LS.main([DB, "t.txt", "v.txt", "ckpt.pt", "--pathCheckpoint", str(tmp_path / "out")] + argv)
    assert not (tmp_path / "out").exists()


def test_several_checkpoints_refused(tmp_path):
    with pytest.raises(SystemExit, match="exactly one"):
        LS.main([DB, "t.txt", "v.txt", "a.pt", "b.pt", "--pathCheckpoint", str(tmp_path / "out")])


def test_ctc_on_encoder_refused_by_criterion():
    from cpc2_amd.criterion import CTCPhoneCriterion
    with pytest.raises(ValueError, match="On encoder"):
        CTCPhoneCriterion(16, 5, True)


def test_update_logs_divides_by_last_batch_index():
    logs = {"locLoss_val": np.asarray([3.0]), "locAcc_val": np.asarray([1.5])}
    out = update_logs(logs, 2)                       # three batches: the sums divided by 2, not 3
    assert out["locLoss_val"][0] == 1.5 and out["locAcc_val"][0] == 0.75
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        one = update_logs({"a": np.asarray([0.5]), "b": np.asarray([0.0])}, 0)
    assert np.isinf(one["a"][0]) and np.isnan(one["b"][0])


def test_criteria_state_dict_keys_match_reference(g21):
    _z, meta = g21
    from cpc2_amd.criterion import CTCPhoneCriterion, PhoneCriterion, SpeakerCriterion
    H = 256
    assert list(PhoneCriterion(H, 41, False).state_dict()) == meta["phone1"]["keys"]
    assert list(PhoneCriterion(H, 41, False, nLayers=2).state_dict()) == meta["phone2"]["keys"]
    assert list(SpeakerCriterion(H, meta["n_speakers"]).state_dict()) == meta["speaker"]["keys"]
    assert list(CTCPhoneCriterion(H, 41, False).state_dict()) == meta["ctc"]["keys"]
    assert CTCPhoneCriterion(H, 41, False).BLANK_LABEL == 41
