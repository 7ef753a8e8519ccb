"""Phone error rate without a GPU: the float32 trie statement of tests/per_oracle.py equals the reference's recorded beam search
(tests/golden/g26_per.npz, tools/make_golden_per.py) bit for bit on every tie-free case and its alignment score on every pair;
the library declares and exports the new entry points and refuses, by name and before any GPU call, what it does not take; the
command-line tool parses its arguments and refuses a run directory that is no CTC probe before it opens any audio."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import per_oracle
from cpc2_amd import _lib, seq_alignment as sa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIE_FREE = ["T1P2k1", "T7P3k1", "T32P9k20", "T32P9k20_blankmid", "T40P70k20_peaky", "T128P42k100_peaky", "T96P42k20_rand",
            "T128P42k20_rand_denormal"]


def recorded(g, tag):
    lens = g[f"{tag}_lens"]
    return [(int(b), [int(x) for x in lab[:n]]) for b, lab, n in zip(g[f"{tag}_score_bits"], g[f"{tag}_labels"], lens)]


def as_bits(out):
    return [(int(np.float32(s).view(np.uint32)), list(lab)) for s, lab in out]


def test_golden_holds_the_cases_of_the_issue(golden):
    g = golden("g26_per.npz")
    meta = json.loads(str(g["meta"]))
    by_name = {c["name"]: c for c in meta["search"]}
    assert [(by_name[n]["T"], by_name[n]["P"], by_name[n]["nKeep"], by_name[n]["blank"]) for n in TIE_FREE] == [
        (1, 2, 1, 1), (7, 3, 1, 2), (32, 9, 20, 8), (32, 9, 20, 3), (40, 70, 20, 69), (128, 42, 100, 41), (96, 42, 20, 41),
        (128, 42, 20, 41)]
    assert all(by_name[n]["tie_free"] for n in TIE_FREE) and not by_name["T6P5k4_tied"]["tie_free"]
    assert by_name["T128P42k20_rand_denormal"]["best"] < 1.1754944e-38          # the denormal range of f32
    assert len(g["al_score_110"]) == 41 and g["al_len2"].min() == 0 and g["al_len1"].min() >= 1
    assert (g["al_len2"] > g["al_len1"]).any() and g["al_score_110"][0] == 0


@pytest.mark.parametrize("name", TIE_FREE)
def test_oracle_equals_the_reference_bit_for_bit(golden, name):
    g = golden("g26_per.npz")
    case = next(c for c in json.loads(str(g["meta"]))["search"] if c["name"] == name)
    out, tie = per_oracle.beam_search(g[f"bs_{name}_probs"], case["nKeep"], case["blank"])
    assert not tie
    assert as_bits(out) == recorded(g, f"bs_{name}")


@pytest.mark.parametrize("tag,n_keep,blank", [("bs_T6P5k4_tied", 4, 4), ("ut_small", 10, 2), ("ut_big", 10, 11)])
def test_oracle_on_tied_cases_differs_only_inside_groups_of_equal_scores(golden, tag, n_keep, blank):
    """The reference orders equal scores by the prefixes' strings, the oracle by (parent rank, symbol): the scores agree as a
    sorted list, and every prefix whose score is unique and above the last kept score is at the same place."""
    g = golden("g26_per.npz")
    out, tie = per_oracle.beam_search(g[f"{tag}_probs"], n_keep, blank)
    assert tie
    mine, ref = as_bits(out), recorded(g, tag)
    assert [b for b, _ in mine] == [b for b, _ in ref]
    counts = {}
    for b, _ in ref:
        counts[b] = counts.get(b, 0) + 1
    for a, b in zip(mine, ref):
        if counts[b[0]] == 1 and b[0] > ref[-1][0]:
            assert a == b
    if tag == "ut_big":
        assert mine[0] == (int(np.float32(1.09).view(np.uint32)), [10])


def test_oracle_stats_describe_the_search_and_do_not_change_it(golden):
    """beam_search(..., stats={}) reports what the input made the search do -- where the cut between the nKeep-th and the next
    candidate falls, groups of equal scores across it, folds, re-entries -- consistently with the returned tie flag, and returns
    what the call without it returns."""
    g = golden("g26_per.npz")
    by_name = {c["name"]: c for c in json.loads(str(g["meta"]))["search"]}
    for name in ("T6P5k4_tied", "T32P9k20_blankmid", "T96P42k20_rand"):
        case, probs = by_name[name], g[f"bs_{name}_probs"]
        plain, tie = per_oracle.beam_search(probs, case["nKeep"], case["blank"])
        stats = {}
        out, tie_s = per_oracle.beam_search(probs, case["nKeep"], case["blank"], stats=stats)
        assert as_bits(out) == as_bits(plain) and tie_s == tie
        assert set(stats) == {"levels", "groups", "folds", "reentries", "rejoined", "max_beam", "nodes"}
        assert set(stats["levels"]) <= {0, 1, 2, 3, "tie"}
        assert stats["levels"].count("tie") == len(stats["groups"])
        assert tie or "tie" not in stats["levels"]              # a tie across the cut is a tie among the first nKeep + 1
        assert stats["max_beam"] == case["nKeep"] and 0 <= stats["rejoined"] <= stats["reentries"]
        # a frame has more candidates than nKeep from the first one that extends more than nKeep / P prefixes on
        assert len(stats["levels"]) >= case["T"] - 2 and stats["nodes"] <= 1 + case["T"] * case["nKeep"]
        for group in stats["groups"]:
            assert 0 < group["need"] < group["size"] <= group["hi"] - group["lo"] + 1
            assert group["lo"] <= group["taken_hi"] < group["hi"] < case["nKeep"] * case["P"]
        if name == "T6P5k4_tied":
            assert tie and stats["groups"] and stats["folds"] > 0
        else:
            assert not tie and not stats["groups"] and "tie" not in stats["levels"] and stats["folds"] > 0
    # by hand: two frames of (0.5, 0.25, 0.25), blank 0, nKeep 2.  Frame 0: "" 0.5, then "1" and "2" at 0.25 -- three candidates,
    # the second and the third equal (slots 1 and 2), one of them taken.  Frame 1 extends "" and "1": "" 0.25, "1" 0.125 + 0.0625
    # + its extension from "" 0.125 (a fold) = 0.3125, "2" 0.125 (it had no node: no re-entry), "12" 0.0625, "11" 0 (pb of "1").
    stats = {}
    out, tie = per_oracle.beam_search(np.array([[0.5, 0.25, 0.25]] * 2, np.float32), 2, 0, stats=stats)
    assert [(float(s), lab) for s, lab in out] == [(0.3125, [1]), (0.25, [])] and tie
    assert stats == dict(levels=["tie", 2], groups=[dict(frame=0, size=2, lo=1, hi=2, need=1, taken_hi=1)], folds=1, reentries=0, rejoined=0,
                         max_beam=2, nodes=2)


def test_oracle_alignment_score_equals_the_reference(golden):
    g = golden("g26_per.npz")
    for i in range(len(g["al_len1"])):
        s1, s2 = g["al_seq1"][i, :g["al_len1"][i]], g["al_seq2"][i, :g["al_len2"][i]]
        assert per_oracle.align_score(s1, s2, -1, -1, 0) == g["al_score_110"][i]
        assert per_oracle.align_score(s1, s2, -2, -3, 1) == g["al_score_231"][i]
        assert per_oracle.get_seq_PER(s1, s2) == g["al_per"][i]
    assert g["al_per"][-1] == 4. / 7.                                            # cpc/unit_tests.py:269-276
    with pytest.raises(ZeroDivisionError):
        per_oracle.get_seq_PER([], [1, 2])


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "cpc2_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("cpc_ctc_beam_search_scratch_bytes", "cpc_ctc_beam_search", "cpc_align_score"):
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in cpc2_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES
    assert _lib.load().cpc_version() >= 116


def test_library_refuses_by_name_before_any_gpu_call():
    lib = _lib.load()
    query = lib.cpc_ctc_beam_search_scratch_bytes
    assert query(1, 128, 42, 100) > 0 and query(64, 128, 128, 128) > 0
    for bad, word in [((1, 128, 42, 129), b"nKeep=129"), ((1, 128, 42, 0), b"nKeep=0"), ((1, 128, 129, 20), b"P=129"),
                      ((1, 128, 1, 20), b"P=1"), ((1, 0, 42, 20), b"t_max=0"), ((0, 8, 42, 20), b"n=0"), ((1, 8193, 42, 20), b"t_max=8193")]:
        assert query(*bad) == 0
        assert word in lib.cpc_last_error(), (bad, lib.cpc_last_error())
    one = ctypes.c_void_p(256)                                                   # never dereferenced: refused before any launch

    def search(p, n_keep, blank, scratch_bytes=1 << 30):
        return lib.cpc_ctc_beam_search(one, one, 1, 8, p, n_keep, blank, 0, one, one, one, one, one, one, scratch_bytes, None)
    assert search(42, 20, 42) == -1 and b"blank=42" in lib.cpc_last_error()
    assert search(42, 20, -1) == -1 and b"blank=-1" in lib.cpc_last_error()
    assert search(42, 129, 41) == -1 and b"nKeep=129" in lib.cpc_last_error()
    assert search(129, 20, 41) == -1 and b"P=129" in lib.cpc_last_error()
    assert search(42, 20, 41, scratch_bytes=16) == -3 and b"scratch" in lib.cpc_last_error()
    assert lib.cpc_align_score(one, 4097, one, one, 8, one, 1, -1, -1, 0, one, None) == -1 and b"4096" in lib.cpc_last_error()
    assert lib.cpc_align_score(one, 8, one, one, 8, one, 0, -1, -1, 0, one, None) == -1
    assert lib.cpc_align_score(one, 8, one, one, 8, one, 1, -1, 1 << 16, 0, one, None) == -1 and b"m=65536" in lib.cpc_last_error()


def test_python_refuses_by_name():
    probs = torch.full((1, 8, 42), 1 / 42.)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sa.beam_search_batch(probs, None, 20, 41)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sa.beam_search(probs[0], 20, 41)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sa.align_score_batch(torch.zeros(1, 4, dtype=torch.int32), torch.tensor([4]), torch.zeros(1, 4, dtype=torch.int32),
                             torch.tensor([4]), -1, -1, 0)
    with pytest.raises(ValueError, match="T = 0"):
        sa.beam_search(np.zeros((0, 42), np.float32), 20, 41)
    with pytest.raises(ValueError, match="T = 0"):
        sa.beam_search_batch(torch.zeros(2, 0, 42), None, 20, 41)
    with pytest.raises(ValueError, match="nKeep=129"):
        sa.beam_search_batch(probs, None, 129, 41)
    with pytest.raises(ValueError, match="P=129"):
        sa.beam_search_batch(torch.zeros(1, 8, 129), None, 20, 41)
    with pytest.raises(ValueError, match=r"blankLabel=42 is outside \[0, P=42\)"):
        sa.beam_search_batch(probs, None, 20, 42)
    with pytest.raises(ValueError, match="blankLabel=-1"):
        sa.beam_search(probs[0], 20, -1)
    with pytest.raises(ZeroDivisionError):
        sa.get_seq_PER([], [1, 2])
    with pytest.raises(ZeroDivisionError):
        sa.NeedlemanWunschAlignScore([], [1, 2], -1, -1, 0)


def test_tool_parses_its_arguments():
    from cpc2_amd.eval import phone_error_rate as per
    a = per.parse_args(["probe"])
    assert (a.pathProbe, a.pathVal, a.pathDB, a.pathPhone, a.nKeep, a.batchSizeGPU, a.debug, a.out) == (
        "probe", None, None, None, 100, None, False, None)
    a = per.parse_args(["probe", "--pathVal", "v.txt", "--pathDB", "db", "--pathPhone", "ph.txt", "--nKeep", "20",
                        "--batchSizeGPU", "4", "--debug", "--out", "o.json"])
    assert (a.pathVal, a.pathDB, a.pathPhone, a.nKeep, a.batchSizeGPU, a.debug, a.out) == ("v.txt", "db", "ph.txt", 20, 4, True,
                                                                                            "o.json")


def _run_args(tmp_path, **changes):
    args = dict(pathDB=str(tmp_path / "no_such_db"), pathTrain="t.txt", pathVal="v.txt", load=["ckpt.pt"], pathPhone="phones.txt",
                CTC=True, pathCheckpoint=str(tmp_path / "checkpoint"), nGPU=1, batchSizeGPU=8, get_encoded=False,
                file_extension=".flac", size_window=20480)
    args.update(changes)
    (tmp_path / "checkpoint_args.json").write_text(json.dumps(args))


@pytest.mark.parametrize("changes,word", [(dict(CTC=False), "--CTC"), (dict(pathPhone=None), "--CTC"),
                                          (dict(get_encoded=True), "--get_encoded")])
def test_tool_refuses_a_run_that_is_no_ctc_probe_before_opening_audio(tmp_path, monkeypatch, changes, word):
    from cpc2_amd.eval import phone_error_rate as per

    def no_audio(*a, **k):
        raise AssertionError("the tool looked for audio before refusing the run")
    monkeypatch.setattr(per, "findAllSeqs", no_audio)
    monkeypatch.setattr(per, "AudioBatchData", no_audio)
    _run_args(tmp_path, **changes)
    with pytest.raises(SystemExit) as e:
        per.main([str(tmp_path)])
    assert word in str(e.value) and str(tmp_path) in str(e.value)


def test_tool_reads_the_run_and_applies_the_overrides(tmp_path):
    from cpc2_amd.eval import phone_error_rate as per
    with pytest.raises(SystemExit, match="checkpoint_args.json"):
        per.load_run(str(tmp_path), per.parse_args([str(tmp_path)]))
    _run_args(tmp_path)
    with pytest.raises(SystemExit, match="no checkpoint_N.pt"):
        per.load_run(str(tmp_path), per.parse_args([str(tmp_path)]))
    for name in ("checkpoint_2.pt", "checkpoint_10.pt", "checkpoint_logs.json", "checkpoint_x.pt"):
        (tmp_path / name).write_text("")
    run, ckpt = per.load_run(str(tmp_path), per.parse_args([str(tmp_path), "--pathVal", "other.txt", "--batchSizeGPU", "4"]))
    assert os.path.basename(ckpt) == "checkpoint_10.pt"
    assert (run.pathVal, run.batchSizeGPU, run.pathPhone, run.size_window) == ("other.txt", 4, "phones.txt", 20480)
