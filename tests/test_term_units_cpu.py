"""Term detection and term discovery on quantized units, the parts that need no GPU: the scratch queries,
the exported names, the refusals of the tools' from_units source, and the statement helper on cases whose answer is written out."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from cpc2_amd import _lib
from cpc2_amd.eval import term_detection as detection_tool
from cpc2_amd.eval import term_discovery as discovery_tool
from tests import term_units_oracle as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cpc_sdtw_units_scratch_bytes", "cpc_sdtw_units", "cpc_local_align_units_scratch_bytes", "cpc_local_align_units")


# --------------------------------------------------------------------------- library
@pytest.mark.parametrize("query,label", [("cpc_sdtw_units_scratch_bytes", b"sdtw_units"),
                                         ("cpc_local_align_units_scratch_bytes", b"local_align_units")])
def test_scratch_queries(query, label):
    """0 when one strip holds every row item; else min(n_seg, 2048) workgroups x 4 waves x 2 buffers x 12 bytes x max_len_col.
    At the same max_len_col that is the dense entry points' scratch at their cap of 8192 workgroups."""
    lib = _lib.load()
    size = getattr(lib, query)
    for n_seg in (1, 100, 2048, 20000):
        for max_len_row in (64, 65):
            for max_len_col in (1, 500):
                want = 0 if max_len_row <= 64 else min(n_seg, 2048) * 4 * 2 * 12 * max_len_col
                assert size(n_seg, max_len_row, max_len_col) == want == U.scratch_bytes(n_seg, max_len_row, max_len_col)
    dense = getattr(lib, query.replace("_units", ""))
    assert size(20000, 65, 500) == dense(20000, 65, 500)
    assert size(0, 65, 500) == 0 and size(5, 65, 0) == 0
    for bad in ((-1, 65, 500), (5, -65, 500), (5, 65, -500)):
        assert size(*bad) == 0
        message = lib.cpc_last_error()
        assert message.startswith(label + b":") and b"negative size" in message, message


def test_header_library_and_bindings_name_the_entry_points():
    header = open(os.path.join(ROOT, "include", "cpc2_hip.h")).read()
    assert "131 = cpc_sdtw_units / cpc_local_align_units" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert _lib.load().cpc_version() >= 131
    sources = set(os.listdir(os.path.join(ROOT, "cpc2_amd", "csrc")))
    assert {"dtw_units_walk.h", "abx_rule.h", "sdtw_rule.h", "lalign_rule.h", "abx_units.hip", "sdtw_units.hip",
            "lalign_units.hip"} <= sources
    read = lambda f: open(os.path.join(ROOT, "cpc2_amd", "csrc", f)).read()  # noqa: E731
    # the recurrences stay in one copy: the rule headers define them, the six kernels include them
    for rule, header_name, users in (("struct AbxRule", "abx_rule.h", ("abx.hip", "abx_units.hip")),
                                     ("struct SdRule", "sdtw_rule.h", ("sdtw.hip", "sdtw_units.hip")),
                                     ("struct LaRule", "lalign_rule.h", ("lalign.hip", "lalign_units.hip"))):
        holders = [f for f in sorted(sources) if rule in read(f)]
        assert holders == [header_name], (rule, holders)
        for user in users:
            assert f'#include "{header_name}"' in read(user), user
    # ... and so does the walk on unit ids: the three unit kernels include it, and the ABX one has no walk of its own left
    for user in ("abx_units.hip", "sdtw_units.hip", "lalign_units.hip"):
        assert '#include "dtw_units_walk.h"' in read(user), user
    abx_units = read("abx_units.hip")
    assert "readlane" not in abx_units and not re.search(r"\bshr1\s*\(", abx_units)
    assert not re.search(r"for\s*\([^)]*\brs\b", abx_units), "a strip loop"
    assert len(re.findall(r"\bfor\s*\(", abx_units)) == 2, "the segment loop and the pair loop"


# --------------------------------------------------------------------------- the tools' refusals
def _detection_argv(tmp_path, *more, units="units.txt"):
    (tmp_path / "q.txt").write_text("q0 utt0 0.10 0.50\n")
    (tmp_path / "r.txt").write_text("q0 utt1\n")
    return ["from_units", str(tmp_path / units), "--queries", str(tmp_path / "q.txt"), "--relevance", str(tmp_path / "r.txt"),
            "--out", str(tmp_path / "out"), *more]


def _discovery_argv(tmp_path, *more, units="units.txt", threshold="0.25"):
    return ["from_units", str(tmp_path / units), "--threshold", threshold, "--out", str(tmp_path / "out"), *more]


def _write_units(tmp_path, name="units.txt"):
    rng = np.random.default_rng(5)
    lines = [f"utt{k}\t" + ",".join(str(u) for u in U.draw_units(rng, 90 + 10 * k, 12)) for k in range(3)]
    (tmp_path / name).write_text("\n".join(lines) + "\n")


def test_detection_from_units_refusals(tmp_path):
    tool = detection_tool
    # --seqNorm is refused before the unit file is looked at: the file does not exist
    with pytest.raises(ValueError, match="--seqNorm"):
        tool.check_args(tool.parse_args(_detection_argv(tmp_path, "--seqNorm", units="missing.txt")))
    with pytest.raises(ValueError, match="--query_dir"):
        tool.check_args(tool.parse_args(_detection_argv(tmp_path, "--query_dir", str(tmp_path), units="missing.txt")))
    with pytest.raises(ValueError, match="from_units .*missing.txt"):
        tool.check_args(tool.parse_args(_detection_argv(tmp_path, units="missing.txt")))
    _write_units(tmp_path)
    with pytest.raises(ValueError, match="--query_units .*missing_q.txt"):
        tool.check_args(tool.parse_args(_detection_argv(tmp_path, "--query_units", str(tmp_path / "missing_q.txt"))))
    for flags, word in ((("--top", "0"), "--top"), (("--feature_size", "0"), "--feature_size"), (("--max_doc_frames", "0"), "--max_doc_frames")):
        with pytest.raises(ValueError, match=word):
            tool.check_args(tool.parse_args(_detection_argv(tmp_path, *flags)))
    (tmp_path / "out").mkdir()
    (tmp_path / "out" / "old.txt").write_text("x")
    with pytest.raises(ValueError, match="--out"):
        tool.check_args(tool.parse_args(_detection_argv(tmp_path, units="missing.txt")))
    (tmp_path / "out" / "old.txt").unlink()
    args = tool.check_args(tool.parse_args(_detection_argv(tmp_path)))
    assert args.load == "from_units" and args.path_units == str(tmp_path / "units.txt") and args.query_units is None
    # the per-penalty layout of segment_quantization: a directory with a quantized_outputs.txt
    penalty = tmp_path / "penalty_2.0"
    penalty.mkdir()
    _write_units(penalty, "quantized_outputs.txt")
    args = tool.check_args(tool.parse_args(_detection_argv(tmp_path, units="penalty_2.0")))
    assert args.path_units == str(penalty / "quantized_outputs.txt")
    # the other sources parse and check as before
    args = tool.check_args(tool.parse_args(["from_pre_computed", str(tmp_path), "--file_extension", ".npy", "--queries",
                                            str(tmp_path / "q.txt"), "--relevance", str(tmp_path / "r.txt"), "--out", str(tmp_path / "out")]))
    assert args.load == "from_pre_computed" and args.query_rows == [("q0", "utt0", 0.10, 0.50)]


def test_discovery_from_units_refusals(tmp_path):
    tool = discovery_tool
    # refused before the unit file is looked at: the file does not exist
    with pytest.raises(ValueError, match="--seqNorm"):
        tool.check_args(tool.parse_args(_discovery_argv(tmp_path, "--seqNorm", units="missing.txt")))
    with pytest.raises(ValueError, match="--threshold q10 with from_units"):
        tool.check_args(tool.parse_args(_discovery_argv(tmp_path, units="missing.txt", threshold="q10")))
    for mode, bad, good in (("cosine", ("0.500001", "0.75", "1e-46"), ("0.5", "0.25", "1e-6")),
                            ("euclidian", ("1.4143", "2"), ("1.4142135", "0.25"))):
        for threshold in bad:                                   # outside (d_same, d_diff]; 1e-46 is 0 in f32
            with pytest.raises(ValueError, match=r"--threshold .*d_same, d_diff"):
                tool.check_args(tool.parse_args(_discovery_argv(tmp_path, "--distance_mode", mode, units="missing.txt", threshold=threshold)))
        for threshold in good:
            with pytest.raises(ValueError, match="from_units .*missing.txt"):
                tool.check_args(tool.parse_args(_discovery_argv(tmp_path, "--distance_mode", mode, units="missing.txt", threshold=threshold)))
    for threshold in ("0", "-1", "nan", "q0", "abc"):
        with pytest.raises(ValueError, match="--threshold"):
            tool.check_args(tool.parse_args(_discovery_argv(tmp_path, units="missing.txt", threshold=threshold)))
    with pytest.raises(ValueError, match="--gap_penalty"):
        tool.check_args(tool.parse_args(_discovery_argv(tmp_path, "--gap_penalty", "-1", units="missing.txt")))
    with pytest.raises(ValueError, match="--max_frames"):               # the kernel's limit: longer utterances cannot be asked for
        tool.check_args(tool.parse_args(_discovery_argv(tmp_path, "--max_frames", "32768", units="missing.txt")))
    (tmp_path / "out").mkdir()
    (tmp_path / "out" / "old.txt").write_text("x")
    with pytest.raises(ValueError, match="--out"):
        tool.check_args(tool.parse_args(_discovery_argv(tmp_path, units="missing.txt")))
    (tmp_path / "out" / "old.txt").unlink()
    _write_units(tmp_path)
    args = tool.check_args(tool.parse_args(_discovery_argv(tmp_path)))
    assert args.load == "from_units" and (args.threshold_kind, args.threshold_value) == ("value", 0.25)
    # the other sources keep qP
    args = tool.check_args(tool.parse_args(["from_pre_computed", str(tmp_path), "--file_extension", ".npy", "--threshold", "q10", "--out",
                                            str(tmp_path / "out")]))
    assert (args.threshold_kind, args.threshold_value) == ("percentile", 10.0)


def test_unit_distances_are_those_of_the_abx_unit_path():
    assert detection_tool.unit_distances("cosine") == (0.0, 0.5)
    assert detection_tool.unit_distances("euclidian") == (0.0, U.SQRT2)


def test_from_units_without_a_gpu_ends_with_no_cpu_fallback(tmp_path, monkeypatch):
    """After the checks, as the other sources do; a refusal still comes first."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    _write_units(tmp_path)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        detection_tool.main(_detection_argv(tmp_path))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        discovery_tool.main(_discovery_argv(tmp_path))
    with pytest.raises(ValueError, match="--seqNorm"):
        discovery_tool.main(_discovery_argv(tmp_path, "--seqNorm"))
    assert not (tmp_path / "out").exists()


def test_python_entry_points_name_a_bad_units_argument():
    from cpc2_amd import term_detection as td
    from cpc2_amd import term_discovery as tdisc
    one = torch.zeros(4, dtype=torch.int32)
    for bad in (torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.float32), torch.zeros(4, 2, dtype=torch.int32),
                torch.zeros(8, dtype=torch.int32)[::2], np.zeros(4, dtype=np.int32)):
        with pytest.raises(TypeError, match="units"):
            td.run_segments_units(bad, one, one, one, one, one, 4, 4, 0.0, 0.5)
        with pytest.raises(TypeError, match="units"):
            td.subsequence_dtw_units(bad, one, one, [0], [1], 0.0, 0.5)
        with pytest.raises(TypeError, match="units"):
            tdisc.run_segments_units(bad, one, one, one, one, one, 4, 4, 0.0, 0.5, 0.25, 0.125)
        with pytest.raises(TypeError, match="units"):
            tdisc.local_alignment_units(bad, one, one, [0, 1], 0.0, 0.5, 0.25, 0.125)
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # a well-formed host tensor: there is no CPU path
        td.run_segments_units(one, one, one, one[:1], one[:2], one[:1], 4, 4, 0.0, 0.5)


# --------------------------------------------------------------------------- the statement on hand-made cases
def test_statement_query_that_occurs_once():
    # 7 8 9 stands at columns 3 .. 5: three cells of distance 0
    score, start, end, length = U.sdtw_units([7, 8, 9], [1, 2, 3, 7, 8, 9, 4, 5], 0.0, 0.5)
    assert (float(score), start, end, length) == (0.0, 3, 5, 3)
    h, span = U.local_align_units([7, 8, 9], [1, 2, 3, 7, 8, 9, 4, 5], 0.0, 0.5, 0.25, 0.125)
    assert (float(h), span) == (0.75, (0, 2, 3, 5, 3))


def test_statement_query_that_occurs_twice_the_first_wins():
    doc = [7, 8, 1, 1, 7, 8, 2]
    score, start, end, length = U.sdtw_units([7, 8], doc, 0.0, 0.5)
    assert (float(score), start, end, length) == (0.0, 0, 1, 2)            # v[1] == v[5] == 0: the first end column
    h, span = U.local_align_units([7, 8], doc, 0.0, 0.5, 0.25, 0.125)
    assert (float(h), span) == (0.5, (0, 1, 0, 1, 2))                      # H = 0.5 at (1, 1) and (1, 5): the smallest j


def test_statement_equal_scores_smallest_i_then_j():
    # the row item holds 5 at rows 1 and 3, the column item at columns 2 and 4: four single cells of H = theta - d_same = 0.25 and
    # nothing longer (5 5 never follows 5 diagonally); the winner is (1, 2)
    h, span = U.local_align_units([1, 5, 2, 5], [3, 4, 5, 6, 5], 0.0, 0.5, 0.25, 0.125)
    assert (float(h), span) == (0.25, (1, 1, 2, 2, 1))
    # nothing in common: no positive cell
    h, span = U.local_align_units([1, 2, 3], [4, 5], 0.0, 0.5, 0.25, 0.125)
    assert (float(h), span) == (0.0, (-1, -1, -1, -1, -1))
    # the subsequence score of a query with no equal unit is d_diff, from the first column, by the shortest path
    score, start, end, length = U.sdtw_units([1, 2, 3], [4, 5], 0.0, 0.5)
    assert (float(score), start, end, length) == (0.5, 0, 0, 3)
    # ties among predecessors go to diag, then left, then up: with all cells equal the path of (2, 2) is the diagonal
    score, start, end, length = U.sdtw_units([1, 1, 1], [1, 1, 1], 0.125, 0.75)
    assert (float(score), start, end, length) == (0.125, 0, 0, 3)          # v[0] == v[1] == v[2]: the first end column (straight up)


def test_a_unit_id_beyond_int32_is_refused_by_the_file_s_name(tmp_path):
    path = tmp_path / "big.txt"
    path.write_text("utt0\t1,2,1099511627776\n")
    with pytest.raises(ValueError, match=r"from_units .*big.txt.*int32"):
        detection_tool.read_units(str(path), "from_units")
    _write_units(tmp_path)
    assert [name for name, _ in detection_tool.read_units(str(tmp_path / "units.txt"), "from_units")] == ["utt0", "utt1", "utt2"]
