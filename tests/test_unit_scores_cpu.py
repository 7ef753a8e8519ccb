"""cpc2_amd.unit_scores' host side and the unit_quality tool without a GPU: hand cases of scores(), the majority-phone ties, the
parsing of a quantized file, every refusal of the tool raised before a file is opened, the skipped / mismatched bookkeeping, and the
C entry points' refusals that need no device."""
import builtins
import math
import os
import re

import numpy as np
import pytest

import unit_scores_oracle as UO
from cpc2_amd import _lib
from cpc2_amd import unit_scores as us
from cpc2_amd.eval import unit_quality as uq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _counts(joint, unit_runs=None, phone_runs=None, boundaries=None, tol=2, has_labels=True):
    joint = np.asarray(joint, dtype=np.int64)
    unit_runs = joint.sum(axis=1) if unit_runs is None else np.asarray(unit_runs, dtype=np.int64)
    phone_runs = joint.sum(axis=0) if phone_runs is None else np.asarray(phone_runs, dtype=np.int64)
    boundaries = np.zeros((0, 5), np.int64) if boundaries is None else np.asarray(boundaries, dtype=np.int64)
    return us.UnitCounts(joint, unit_runs, phone_runs, np.zeros(1, np.int64), boundaries, tol, has_labels)


def _against_oracle(c, feature_size=0.01):
    got = us.scores(c, feature_size)
    want, bound = UO.scores(c.joint, c.unit_runs, c.phone_runs, c.boundaries, c.tol, feature_size, c.has_labels)
    UO.assert_scores_close(got, want, bound)
    return got, bound


def test_diagonal_joint_is_pure():
    got, bound = _against_oracle(_counts(np.diag([5, 9, 2, 16])))
    assert got["phone_purity"] == 1.0 and got["cluster_purity"] == 1.0
    assert abs(got["pnmi"] - 1.0) <= bound["pnmi"] and abs(got["MI"] - got["H_phone"]) <= bound["MI"] + bound["H_phone"]
    assert got["used_units"] == 4 and got["n_frames"] == 32


def test_outer_product_joint_has_no_information():
    """joint[z][y] = a[z] b[y]: p(y, z) = p(y) p(z) exactly, every ratio is exactly 1 and its logarithm exactly 0."""
    a, b = np.array([1, 2, 5, 3]), np.array([4, 1, 7])
    got, bound = _against_oracle(_counts(np.outer(a, b)))
    assert abs(got["MI"]) <= bound["MI"] and got["MI"] == 0.0 and got["pnmi"] == 0.0
    assert got["phone_purity"] == 7 / 12 and got["cluster_purity"] == 5 / 11


def test_one_phone_only_gives_nan_pnmi():
    got, _ = _against_oracle(_counts([[3], [4], [1]]))
    assert got["H_phone"] == 0.0 and math.isnan(got["pnmi"]) and got["MI"] == 0.0
    assert got["phone_purity"] == 1.0 and got["cluster_purity"] == 0.5


def test_worked_bitrate_example():
    """Two units, 4 frames each, 8 frames of 10 ms: H = 1 bit, 8 * 1 / 0.08 = 100 bits/s by frames.  Runs: unit 0 in 1 run, unit 1 in
    3: H_runs = 2 - 0.75 log2 3 = 0.8112781..., 4 runs in 0.08 s: 40.56... bits/s; a mean run of 2 frames."""
    got, bound = _against_oracle(_counts([[4, 0], [0, 4]], unit_runs=[1, 3], phone_runs=[2, 2]))
    assert got["H_unit"] == 1.0 and got["perplexity"] == 2.0 and got["bitrate_frames"] == 100.0
    h_runs = 2 - 0.75 * math.log2(3)
    # (the hand formula has its own roundings: a logarithm, two products, a difference and a division, each u relative of <= 41)
    assert abs(got["bitrate_runs"] - 4 * h_runs / 0.08) <= bound["bitrate_runs"] + 6 * UO.U53 * 41
    assert got["mean_unit_run"] == 2.0 and got["mean_phone_run"] == 2.0
    other, _ = _against_oracle(_counts([[4, 0], [0, 4]], unit_runs=[1, 3], phone_runs=[2, 2]), feature_size=0.02)
    assert other["bitrate_frames"] == 50.0


def test_unit_never_used():
    got, _ = _against_oracle(_counts([[3, 1], [0, 0], [2, 6]], unit_runs=[2, 0, 3]))
    assert got["used_units"] == 2 and got["n_units"] == 3
    assert [row[0] for row in us.unit_to_phone(_counts([[3, 1], [0, 0], [2, 6]]))] == [0, 2]


def test_random_joint_within_the_derived_bound():
    rs = np.random.RandomState(3)
    joint = rs.randint(0, 50, size=(37, 11)) * (rs.rand(37, 11) < 0.6)
    rows = rs.randint(0, 40, size=(6, 5))
    got, bound = _against_oracle(_counts(joint, unit_runs=rs.randint(1, 30, size=37), phone_runs=rs.randint(1, 90, size=11),
                                         boundaries=rows))
    assert all(0 <= b < 1e-12 for b in bound.values())
    assert got["boundaries"]["n_ref"] == int(rows[:, 0].sum())


def test_without_labels_only_the_unit_side():
    got, _ = _against_oracle(_counts([[3], [5]], has_labels=False))
    assert "pnmi" not in got and "phone_purity" not in got and "boundaries" not in got
    assert {"H_unit", "perplexity", "bitrate_frames", "bitrate_runs", "mean_unit_run", "used_units", "n_units"} <= set(got)


def test_scores_refuse_nothing_counted_and_bad_feature_size():
    with pytest.raises(ValueError, match="no frame"):
        us.scores(_counts(np.zeros((2, 2))))
    with pytest.raises(ValueError, match="feature_size"):
        us.scores(_counts([[1]]), feature_size=0.0)


def test_majority_phone_ties_go_to_the_lowest_index():
    joint = [[2, 5, 5, 1], [0, 0, 0, 0], [7, 7, 7, 7], [0, 1, 0, 1]]
    got = us.unit_to_phone(_counts(joint))
    assert got == UO.unit_to_phone(joint)
    assert [(z, y, c) for z, y, c, _t, _p in got] == [(0, 1, 5), (2, 0, 7), (3, 1, 1)]
    assert got[0][3] == 13 and got[0][4] == 5 / 13


# ----------------------------------------------------------------------------- the tool
def test_read_quantized(tmp_path):
    path = tmp_path / "quantized_outputs.txt"
    path.write_text("a/b/utt1.flac\t3,3,0,12\nutt2\t7\nutt3\t")                  # (no trailing newline, as the writer leaves it)
    got = uq.read_quantized(str(path))
    assert [n for n, _u in got] == ["utt1", "utt2", "utt3"]
    assert got[0][1].tolist() == [3, 3, 0, 12] and got[1][1].tolist() == [7] and got[2][1].tolist() == []
    assert got[0][1].dtype == np.int32


def test_read_quantized_refuses_group_tokens_by_name(tmp_path):
    path = tmp_path / "quantized_outputs.txt"
    path.write_text("utt1\t3,3\nspk-utt2\t65-241,3-4\n")
    with pytest.raises(ValueError, match=r"line 2 \(spk-utt2\).*'65-241'.*several unit groups"):
        uq.read_quantized(str(path))


MISSING = os.path.join(ROOT, "no", "such", "place")
QUANT = ["--quantized", os.path.join(MISSING, "quantized_outputs.txt")]
REFUSED = [
    (["--out", ROOT] + QUANT, ValueError, "--out .* not an empty directory"),
    (["--out", MISSING] + QUANT + ["--clustering", "c.pt", "--path_audio_data", MISSING], ValueError, "exactly one"),
    (["--out", MISSING], ValueError, "exactly one"),
    (["--out", MISSING, "--clustering", "c.pt"], ValueError, "--path_audio_data"),
    (["--out", MISSING, "--clustering", "c.pt", "--path_audio_data", MISSING, "--file_extension", ".mp3"], NotImplementedError, "mp3"),
    (["--out", MISSING, "--feature_size", "0"] + QUANT, ValueError, "--feature_size"),
    (["--out", MISSING, "--feature_size", "-0.01"] + QUANT, ValueError, "--feature_size"),
    (["--out", MISSING, "--tolerance", "-1"] + QUANT, ValueError, "--tolerance"),
    (["--out", MISSING, "--max_length_mismatch", "-1"] + QUANT, ValueError, "--max_length_mismatch"),
    (["--out", MISSING, "--n_units", "0"] + QUANT, ValueError, "--n_units"),
    (["--out", MISSING, "--n_units", "16385"] + QUANT, ValueError, "--n_units"),
    (["--out", MISSING, "--n_phones", "0", "--pathPhone", "p.txt"] + QUANT, ValueError, "--n_phones"),
    (["--out", MISSING, "--n_phones", "1025", "--pathPhone", "p.txt"] + QUANT, ValueError, "--n_phones"),
]


@pytest.mark.parametrize("argv,error,text", REFUSED, ids=[" ".join(a for a in r[0] if a.startswith("--")) + f" #{i}"
                                                          for i, r in enumerate(REFUSED)])
def test_tool_refuses_before_a_file_is_opened(argv, error, text, monkeypatch):
    opened = []
    real_open = builtins.open

    def watched(file, *a, **k):
        opened.append(file)
        return real_open(file, *a, **k)

    monkeypatch.setattr(builtins, "open", watched)
    monkeypatch.setattr(uq, "findAllSeqs", lambda *a, **k: opened.append(a) or ([], []))
    monkeypatch.setattr(uq, "parseSeqLabels", lambda *a, **k: opened.append(a) or ({}, 1))
    monkeypatch.setattr(uq, "read_quantized", lambda *a, **k: opened.append(a) or [])
    with pytest.raises(error, match=text):
        uq.main(argv)
    assert not opened and not os.path.exists(MISSING)


def test_skipped_and_mismatched_bookkeeping():
    names = ["a", "b", "c", "d", "e", "f"]
    unit_lengths = [100, 50, 30, 0, 12, 9]
    labels = {"a": [0] * 102, "b": [0] * 47, "d": [0] * 2, "e": [0] * 10, "f": [0] * 9, "zz": [1]}
    kept, skipped, mismatched = uq.pair_lengths(names, unit_lengths, labels, 2)
    assert kept == [(0, 100), (3, 0), (4, 10), (5, 9)]                   # the first min(frames, labels) frames
    assert skipped == ["c"]
    assert mismatched == [{"name": "b", "frames": 50, "labels": 47}]
    kept, skipped, mismatched = uq.pair_lengths(names, unit_lengths, labels, 0)
    assert [i for i, _n in kept] == [5] and [m["name"] for m in mismatched] == ["a", "b", "d", "e"]
    kept, skipped, mismatched = uq.pair_lengths(names, unit_lengths, None, 2)
    assert kept == list(enumerate(unit_lengths)) and not skipped and not mismatched


# ----------------------------------------------------------------------------- the C ABI, host side
def test_entry_points_are_declared_and_sized():
    header = open(os.path.join(ROOT, "include", "cpc2_hip.h")).read()
    declared = set(re.findall(r"\b(cpc_unit_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == {"cpc_unit_counts", "cpc_unit_boundaries", "cpc_unit_counts_scratch_bytes", "cpc_unit_boundaries_scratch_bytes",
                        "cpc_unit_counts_lds_cells", "cpc_unit_counts_chunk"}
    for name in declared:
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.cpc_version() >= 126
    assert lib.cpc_unit_counts_lds_cells() == 16384 and lib.cpc_unit_counts_chunk() == 4096
    assert lib.cpc_unit_counts_scratch_bytes(1000) >= 8 * 1001
    assert lib.cpc_unit_boundaries_scratch_bytes(1000, 5000) >= 8 * 1001 + 2 * 4 * 5000
    assert lib.cpc_unit_counts_scratch_bytes(-1) == 0 and b"unit_counts" in lib.cpc_last_error()
    assert lib.cpc_unit_counts_scratch_bytes((1 << 20) + 1) == 0
    assert lib.cpc_unit_boundaries_scratch_bytes(4, -1) == 0 and b"unit_boundaries" in lib.cpc_last_error()
    assert us.MAX_UNITS == 16384 and us.MAX_PHONES == 1024


def test_count_refuses_host_tensors():
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        us.count(torch.zeros(4, dtype=torch.int32), None, torch.zeros(1, dtype=torch.int64), None, torch.tensor([4], dtype=torch.int32),
                 2, 1)
