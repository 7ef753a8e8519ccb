"""CTC forced alignment without a GPU: the float64 statement of tests/ctc_align_oracle.py against a brute-force enumeration of
all label strings, seq_alignment.frame_labels and the writers of `common_voices_eval align` on hand-made paths, the
sub-command's parser and its refusal of a non-empty output directory, and the library's declaration of the new entry points
with their refusals outside each limit."""
import argparse
import itertools
import json
import os

import numpy as np
import pytest

import ctc_align_oracle as oracle
from cpc2_amd import _lib
from cpc2_amd.dataset import parseSeqLabels
from cpc2_amd.eval import common_voices_eval as cv
from cpc2_amd.seq_alignment import AlignResult, frame_labels, head_frame_of, head_tokens

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISSING = os.path.join(ROOT, "tests", "golden", "no_such_directory")


# ----------------------------------------------------------------------------- the statement against an enumeration
def _brute(logits, y, blank):
    """The largest logit sum over all k^T label strings that collapse to y (-inf when none does), and whether two reach it."""
    t_len, k = logits.shape
    best, count = -np.inf, 0
    for seq in itertools.product(range(k), repeat=t_len):
        if oracle.collapse(seq, blank) == list(y):
            total = 0.0
            for t, a in enumerate(seq):
                total += float(logits[t, a])
            if total > best:
                best, count = total, 1
            elif total == best:
                count += 1
    return best, count


def test_statement_equals_the_enumeration_of_all_label_strings():
    rng = np.random.default_rng(0)
    aligned = tied = impossible = 0
    for trial in range(300):
        k, t_len, n_lab = int(rng.integers(2, 4)), int(rng.integers(1, 7)), int(rng.integers(0, 4))
        blank = k - 1
        y = [int(v) for v in rng.integers(0, k - 1, n_lab)]
        zero = trial % 3 == 0
        logits = np.zeros((t_len, k), np.float32) if zero else rng.standard_normal((t_len, k)).astype(np.float32)
        res = oracle.align(logits, t_len, y)
        best, count = _brute(logits, y, blank)
        need = oracle.needed_frames(y)
        assert (res["status"] == 1) == (best == -np.inf) == (t_len < need), (t_len, y)          # the existence condition
        if res["status"] == 1:
            assert (res["path"] == -1).all() and np.isnan(res["score"]).all()
            impossible += 1
            continue
        assert res["status"] == 0
        labels = oracle.labels_of(res["path"], y, blank)
        assert oracle.collapse(labels, blank) == y                                               # a path of the target
        assert res["score"][0] == best                       # and a best one (the same additions in the same order: the same bits)
        assert res["ties"] == int(count >= 2)                # a label string is one state path: a tie on the path is a second best string
        if zero and n_lab >= 1 and t_len > need:
            assert res["ties"] == 1                                                              # a frame to spare: a tie
            tied += 1
        for i in range(n_lab):
            frames = np.nonzero(res["path"] == 2 * i + 1)[0]
            assert (res["first"][i], res["last"][i]) == (frames[0], frames[-1])
        aligned += 1
    assert aligned >= 150 and tied >= 10 and impossible >= 20, (aligned, tied, impossible)


def test_statement_status_and_ties():
    logits = np.zeros((3, 4), np.float32)
    assert oracle.align(logits, 0, [])["status"] == 1                   # no frame to start from
    assert oracle.align(logits, 2, [1, 1])["status"] == 1               # a repeat needs a blank between
    three = oracle.align(logits, 3, [1, 1])
    assert three["status"] == 0 and list(three["path"]) == [1, 2, 3] and three["ties"] == 0
    assert oracle.align(logits, 4, [1], t_max=3)["status"] == 2
    assert oracle.align(logits, 3, [3])["status"] == 2                  # the blank is no label
    assert oracle.align(logits, 3, [-1])["status"] == 2
    assert oracle.align_batch(logits[None], [3], [[1, 1]], [3])[0]["status"] == 2
    empty = oracle.align(logits, 3, [])
    assert empty["status"] == 0 and list(empty["path"]) == [0, 0, 0] and empty["ties"] == 0 and empty["score"][0] == 0
    # the end prefers the blank and, walking back, staying wins over advancing: with all-zero logits the token comes first
    late = oracle.align(logits, 3, [0])
    assert list(late["path"]) == [1, 2, 2] and late["ties"] == 1
    assert np.isclose(late["score"][1], -3 * np.log(4)) and late["conf"][0] == np.float32(-np.log(4))


# ----------------------------------------------------------------------------- the frame map
def _rows(path, labels):
    return argparse.Namespace(path=np.asarray(path, np.int32), labels=np.asarray(labels, np.int64))


def test_head_frame_of_is_the_nearest_receptive_field_centre():
    assert list(head_frame_of(12, 3)) == [0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2]            # (f - 2) // 4, clamped at both ends
    assert list(head_frame_of(16, 3)) == [0] * 6 + [1] * 4 + [2] * 6                     # the last head frame takes the rest
    assert list(head_frame_of(5, 2, kernel=4, stride=2)) == [0, 0, 0, 1, 1]              # (f - 1) // 2
    assert len(head_frame_of(0, 3)) == 0
    # nearest centre: head frame j covers feature frames 4 j .. 4 j + 7, centre 4 j + 3.5
    for f in range(40):
        j = int(head_frame_of(40, 9)[f])
        assert abs(f - (4 * j + 3.5)) == min(abs(f - (4 * i + 3.5)) for i in range(9)), f


def test_frame_labels_on_hand_made_paths():
    blank = 9
    # tokens 5, 5, 7: states 0 1 1 2 3 4 5 6 (a leading blank, a blank run between the repeats, a trailing blank), then padding
    path = [[0, 1, 1, 2, 3, 4, 5, 6, -1, -1]]
    labels = [[blank, 5, 5, blank, 5, blank, 7, blank, -1, -1]]
    assert list(head_tokens(path[0])) == [0, 0, 0, 0, 1, 1, 2, 2]
    got = frame_labels(_rows(path, labels), [33])[0]
    head = [5, 5, 5, 5, 5, 5, 7, 7]
    assert list(got) == [head[min(max((f - 2) // 4, 0), 7)] for f in range(33)]
    assert list(got[:6]) == [5] * 6 and got[32] == 7 and got.dtype == np.int64          # f < 2 and the last head frame
    with_blank = frame_labels(_rows(path, labels), [33], blank_label=40)[0]
    head = [40, 5, 5, 40, 5, 40, 7, 40]
    assert list(with_blank) == [head[min(max((f - 2) // 4, 0), 7)] for f in range(33)]
    # L = 0: no frame labels without blank_label
    empty = _rows([[0, 0, 0, -1]], [[blank, blank, blank, -1]])
    assert frame_labels(empty, [12]) == [None] and head_tokens(empty.path[0]) is None
    assert list(frame_labels(empty, [12], blank_label=40)[0]) == [40] * 12
    # no alignment: nothing either way; and a batch keeps its order
    both = _rows([[-1, -1, -1, -1], [1, 1, 2, -1]], [[-1, -1, -1, -1], [3, 3, blank, -1]])
    got = frame_labels(both, [8, 12], blank_label=40)
    assert got[0] is None and list(got[1]) == [3] * 10 + [40] * 2
    got = frame_labels(both, [8, 12])
    assert got[0] is None and list(got[1]) == [3] * 12
    # torch tensors are accepted as they are
    import torch
    res = AlignResult(torch.tensor(path, dtype=torch.int32), torch.tensor(labels), *[None] * 7)
    assert list(frame_labels(res, [33])[0]) == list(frame_labels(_rows(path, labels), [33])[0])


# ----------------------------------------------------------------------------- the writers
def test_written_frames_are_read_back_by_parseSeqLabels(tmp_path):
    blank = 9
    path = np.array([0, 1, 1, 2, 3, 4, 5, 6, -1, -1])
    labels = np.array([blank, 5, 5, blank, 5, blank, 7, blank, -1, -1])
    conf = np.array([-0.5, -0.25, -1.0, np.nan])
    n_samples = 33 * 160 + 77
    frames, segments = cv.utterance_alignment(path, labels, conf, n_samples)
    assert len(frames) == 33
    assert [s[0] for s in segments] == [5, 5, 7] and [s[3] for s in segments] == [-0.5, -0.25, -1.0]
    assert segments[0][1] == 0 and segments[-1][2] == n_samples / 16000
    assert all(segments[i][2] == segments[i + 1][1] for i in range(2))                      # they tile [0, duration)
    assert [round(s[1] * 100) for s in segments] == [0, 18, 26]          # head frames 4 and 6 start at feature frames 18 and 26
    none = cv.utterance_alignment(np.array([0, 0, -1]), np.array([blank, blank, -1]), np.zeros(0), 1300)
    assert none == (None, [])
    blanks, no_segments = cv.utterance_alignment(np.array([0, 0, -1]), np.array([blank, blank, -1]), np.zeros(0), 1300, blank_label=40)
    assert list(blanks) == [40] * 8 and no_segments == []
    with open(tmp_path / "alignment_frames.txt", "w") as ff, open(tmp_path / "alignment_segments.txt", "w") as sf:
        cv.write_alignment(ff, sf, "utt-a", frames, segments)
        cv.write_alignment(ff, sf, "utt-b", *none)
        cv.write_alignment(ff, sf, "utt-c", blanks, no_segments)
    parsed, n_phones = parseSeqLabels(str(tmp_path / "alignment_frames.txt"))
    assert parsed["step"] == 160 and set(parsed) == {"step", "utt-a", "utt-c"} and n_phones == 41
    assert parsed["utt-a"] == [int(v) for v in frames] and len(parsed["utt-a"]) == n_samples // 160
    lines = [ln.split() for ln in open(tmp_path / "alignment_segments.txt")]
    assert [ln[:2] for ln in lines] == [["utt-a", "5"], ["utt-a", "5"], ["utt-a", "7"]]
    assert lines[0][2] == "0.000000" and lines[0][3] == lines[1][2] and lines[1][3] == lines[2][2]
    assert abs(float(lines[2][3]) - n_samples / 16000) <= 1e-6 and float(lines[1][4]) == -0.25


def test_parse_transcripts_keeps_empty_transcriptions(tmp_path):
    with open(tmp_path / "t.txt", "w") as f:
        f.write("a 1 2 3\nb\n\nc 0\n")
    assert cv.parse_transcripts(str(tmp_path / "t.txt")) == {"a": [1, 2, 3], "b": [], "c": [0]}


# ----------------------------------------------------------------------------- command line
def test_align_flags():
    assert vars(cv.parse_args(["align", "OUT", "-o", "A"])) == dict(
        command="align", output="OUT", align_dir="A", batchSize=8, debug=False, pathDB=None, pathVal=None, pathPhone=None,
        file_extension=".wav", blank_label=None, name="0")
    args = cv.parse_args(["align", "OUT", "-o", "A", "--batchSize", "2", "--debug", "--pathDB", "D", "--pathVal", "V", "--pathPhone", "P",
                          "--file_extension", ".flac", "--blank_label", "40", "--name", "t"])
    assert (args.batchSize, args.debug, args.pathDB, args.pathVal, args.pathPhone, args.file_extension, args.blank_label, args.name) == (
        2, True, "D", "V", "P", ".flac", 40, "t")
    with pytest.raises(SystemExit):
        cv.parse_args(["align", "OUT"])                                  # the alignment directory is required
    # train and per parse as before
    assert cv.parse_args(["per", "OUT"]).name == "0" and cv.parse_args(["train", "DB", "P", "C"]).output == "out"


def test_align_refuses_a_non_empty_directory_before_anything_is_read(monkeypatch, tmp_path):
    listed = []
    monkeypatch.setattr(cv, "findAllSeqs", lambda *a, **k: listed.append(a) or ([], []))
    run = tmp_path / "run"
    run.mkdir()
    with open(run / "args_training.json", "w") as f:
        json.dump(dict(pathDB=MISSING, file_extension=".flac", pathPhone=MISSING, pathVal=None, pathCheckpoint="CKPT",
                       no_pretraining=False), f)
    full = tmp_path / "full"
    full.mkdir()
    (full / "something.txt").write_text("x")
    with pytest.raises(ValueError, match="exists and is not empty"):
        cv.main(["align", str(run), "-o", str(full)])
    with pytest.raises(ValueError, match="exists and is not empty"):
        cv.main(["align", str(run), "-o", str(full / "something.txt")])
    assert not listed and not (run / "logs_align_0.txt").exists() and os.listdir(full) == ["something.txt"]
    cv.check_align_dir(str(tmp_path / "new"))                            # a new one and an empty one pass
    (tmp_path / "empty").mkdir()
    cv.check_align_dir(str(tmp_path / "empty"))
    # an mp3 run is refused by name as `per` refuses it, before the data set is listed
    with open(run / "args_training.json", "w") as f:
        json.dump(dict(pathDB=MISSING, file_extension=".mp3", pathPhone=MISSING, pathVal=None, pathCheckpoint="CKPT",
                       no_pretraining=False), f)
    with pytest.raises(ValueError, match=r"--file_extension \.mp3"):
        cv.main(["align", str(run), "-o", str(tmp_path / "new")])
    assert not listed and not (tmp_path / "new").exists()


# ----------------------------------------------------------------------------- the library
def test_library_declares_the_aligner():
    lib = _lib.load()
    assert lib.cpc_version() >= 120
    for name in ("cpc_ctc_align_scratch_bytes", "cpc_ctc_align", "cpc_ctc_align_segments"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "cpc2_hip.h")).read()
    assert "torchaudio.functional.forced_align" in header and "UNMEASURED" in header


def test_scratch_query_is_zero_with_a_message_outside_each_limit():
    lib = _lib.load()
    assert lib.cpc_ctc_align_scratch_bytes(1, 1, 0) == 256 + 256
    # f64 [b][t_max] and one byte per (frame, state), each rounded up to 256 bytes
    assert lib.cpc_ctc_align_scratch_bytes(3, 37, 9) == 1024 + (3 * 37 * 19 + 255) // 256 * 256
    assert lib.cpc_ctc_align_scratch_bytes(2, 4096, 1024) == 2 * 4096 * 8 + 2 * 4096 * 2049
    assert lib.cpc_ctc_align_scratch_bytes(65535, 1, 1) > 0
    for bad in [(0, 10, 2), (65536, 10, 2), (1, 0, 0), (1, 4097, 2), (1, 10, -1), (1, 10, 11), (1, 4096, 1025)]:
        assert lib.cpc_ctc_align_scratch_bytes(*bad) == 0, bad
        message = lib.cpc_last_error().decode()
        assert message.startswith("ctc_align:") and f"b={bad[0]} t_max={bad[1]} max_l={bad[2]}" in message, message
