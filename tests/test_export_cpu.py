"""CPU-side checks of the feature export (cpc2_amd/eval/build_zeroSpeech_features.py, cpc2_amd/text.py, csrc/text_digits.h):
the integer statement of the float-to-text conversion equals CPython's repr, the arithmetic the kernels run equals it too when
compiled for the host, and the tool has the reference's command line, its refusals and its time column."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import text_oracle as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANDOM = 200_000


@pytest.fixture(scope="module")
def patterns():
    bits = np.concatenate([T.fixed_patterns(), T.random_patterns(RANDOM, seed=20261017)])
    return bits, T.repr_of(bits)


def test_fixed_list_covers_what_it_names():
    texts = dict(zip(T.fixed_patterns().tolist(), T.repr_of(T.fixed_patterns())))
    assert texts[0x80000000] == "-0.0" and texts[0x00000001] == "1.401298464324817e-45"
    assert texts[0x00800000] == "1.1754943508222875e-38" and len(texts[0x80800000]) == 23
    assert texts[0x7f7fffff] == "3.4028234663852886e+38" and texts[0xff800000] == "-inf" and texts[0xffc00000] == "nan"
    assert texts[T.bits_of(1e-4)] == "9.999999747378752e-05" and texts[T.bits_of(1e16)] == "1.0000000272564224e+16"
    assert texts[T.bits_of(9.99e15)] == "9990000514957312.0" and texts[T.bits_of(16777216.0)] == "16777216.0"
    assert texts[0xc2ce6f44] == "-103.21731567382812"


def test_oracle_equals_repr(patterns):
    bits, want = patterns
    bad = [(hex(b), w, T.format_bits(int(b))) for b, w in zip(bits, want) if T.format_bits(int(b)) != w]
    assert not bad, bad[:10]


# ----------------------------------------------------------------------------- the kernels' arithmetic, compiled for the host
@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    cxx = next((c for c in ("g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler"
    so = tmp_path_factory.mktemp("text_host") / "libtext_host.so"
    subprocess.run([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(so), os.path.join(ROOT, "tests", "text_host.cpp")],
                   check=True)
    lib = ctypes.CDLL(str(so))
    for fn in (lib.text_host_f32, lib.text_host_digits8, lib.text_host_i64):
        fn.restype = ctypes.c_long
    return lib


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _texts(slots, lens):
    for i in range(len(lens)):
        assert not slots[i, lens[i]:].any(), "bytes behind the text"
    return [bytes(slots[i, :lens[i]]).decode() for i in range(len(lens))]


def test_device_arithmetic_on_the_host_equals_repr(host_lib, patterns):
    """format_f32_bits of text_digits.h -- 4-word numbers where they suffice, 8-word ones elsewhere -- with every carry that the
    fixed word counts assume to be zero counted: none may occur, and the bytes are repr's."""
    bits, want = patterns
    bits = np.ascontiguousarray(bits)
    slots, lens = np.zeros((len(bits), 24), np.uint8), np.zeros(len(bits), np.uint8)
    assert host_lib.text_host_f32(_ptr(bits), ctypes.c_long(len(bits)), _ptr(slots), _ptr(lens)) == 0
    got = _texts(slots, lens)
    bad = [(hex(b), w, g) for b, w, g in zip(bits, want, got) if w != g]
    assert not bad, bad[:10]
    assert int(lens.max()) == 23


def test_eight_word_path_alone_gives_the_same_digits(host_lib, patterns):
    bits = np.ascontiguousarray(patterns[0][:20_000 + len(T.fixed_patterns())])
    n = len(bits)
    lo, hi, nd, k = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    assert host_lib.text_host_digits8(_ptr(bits), ctypes.c_long(n), _ptr(lo), _ptr(hi), _ptr(nd), _ptr(k)) == 0
    for i, b in enumerate(bits.tolist()):
        mag = b & 0x7fffffff
        if mag == 0 or mag >= 0x7f800000:
            continue
        digits, kk = T.digits_f32(mag)
        got = [(int(lo[i]) >> (4 * j)) & 15 if j < 16 else int(hi[i]) for j in range(int(nd[i]))]
        assert (got, int(k[i])) == (digits, kk), hex(b)


def test_integer_text_on_the_host(host_lib):
    values = np.array([0, 1, -1, 9, 10, -10, 99, 100, 2 ** 31, -2 ** 31, 10 ** 18, 2 ** 63 - 1, -2 ** 63 + 1, -2 ** 63] +
                      [10 ** p for p in range(19)] + [10 ** p - 1 for p in range(1, 19)], dtype=np.int64)
    slots, lens = np.zeros((len(values), 24), np.uint8), np.zeros(len(values), np.uint8)
    assert host_lib.text_host_i64(_ptr(values), ctypes.c_long(len(values)), _ptr(slots), _ptr(lens)) == 0
    assert _texts(slots, lens) == [str(int(v)) for v in values]


# ----------------------------------------------------------------------------- the Python face without a device
def test_format_rows_refuses_other_types_and_the_host():
    from cpc2_amd.text import format_rows
    for bad in (torch.zeros(2, 2, dtype=torch.float64), torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.float16),
                np.zeros((2, 2), np.float32)):
        with pytest.raises(TypeError, match="float32 or an int64"):
            format_rows(bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        format_rows(torch.zeros(2, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        format_rows(torch.zeros(0, 2, dtype=torch.int64))


# ----------------------------------------------------------------------------- the tool's command line
def test_parser_has_the_reference_flags_and_defaults():
    from cpc2_amd.eval.build_zeroSpeech_features import parse_args
    args = vars(parse_args(["db", "out", "ckpt.pt"]))
    assert args == dict(pathDB="db", pathOut="out", pathCheckpoint="ckpt.pt", extension=".wav", addCriterion=False, oneHot=False,
                        maxSizeSeq=64000, train_mode=False, format="fea", strict=False, dimReduction=None, centroidLimits=None,
                        getEncoded=False, clusters=None, seqNorm=False)
    assert list(args) == ["pathDB", "pathOut", "pathCheckpoint", "extension", "addCriterion", "oneHot", "maxSizeSeq", "train_mode",
                          "format", "strict", "dimReduction", "centroidLimits", "getEncoded", "clusters", "seqNorm"]
    full = parse_args(["db", "out", "c.pt", "--extension", ".flac", "--addCriterion", "--oneHot", "--maxSizeSeq", "32000", "--train_mode",
                       "--format", "af", "--strict", "--dimReduction", "pca.pt", "--centroidLimits", "3", "9", "--getEncoded",
                       "--clusters", "k.pt", "--seqNorm"])
    assert (full.extension, full.maxSizeSeq, full.format, full.dimReduction, full.centroidLimits, full.clusters) == \
        (".flac", 32000, "af", "pca.pt", [3, 9], "k.pt")
    assert full.addCriterion and full.oneHot and full.train_mode and full.strict and full.getEncoded and full.seqNorm
    for fmt in ("fea", "npz", "npy", "af"):
        assert parse_args(["db", "out", "c.pt", "--format", fmt]).format == fmt
    with pytest.raises(SystemExit):
        parse_args(["db", "out", "c.pt", "--format", "txt"])


@pytest.mark.parametrize("flags,name", [(["--format", "af"], "--format af"), (["--addCriterion"], "--addCriterion"),
                                        (["--dimReduction", "pca.pt"], "--dimReduction"),
                                        (["--centroidLimits", "1", "5"], "--centroidLimits")])
def test_refusals_name_their_flag_before_anything_is_written(tmp_path, flags, name):
    from cpc2_amd.eval.build_zeroSpeech_features import main
    out = tmp_path / "features"
    ckpt = os.path.join(ROOT, "tests", "golden", "ref_checkpoint", "checkpoint_7.pt")
    with pytest.raises(NotImplementedError) as err:
        main([os.path.join(ROOT, "tests", "golden", "test_db"), str(out), ckpt, "--extension", ".flac"] + flags)
    assert name in str(err.value)
    assert not out.exists() and not (tmp_path / "features.json").exists() and os.listdir(tmp_path) == []


def test_time_column_is_the_reference_expression():
    from cpc2_amd.eval.build_zeroSpeech_features import frame_times
    stepSize = 160 / 16000
    startStep = stepSize / 2
    want = [str(startStep + step * stepSize) for step in range(400)]
    got = [str(t) for t in frame_times(400, stepSize)]
    assert got == want
    assert got[:3] == ["0.005", "0.015", "0.025"] and got[3] == str(0.005 + 3 * 0.01) and got[399] == str(0.005 + 399 * 0.01)
    assert any(len(t) > 6 for t in got)                    # (the doubles' own digits show: nothing rounds the column)
    assert frame_times(0, stepSize) == []
