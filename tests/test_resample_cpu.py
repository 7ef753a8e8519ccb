"""Sample-rate conversion without a GPU: the library's plan and table against the fp64 statement of tests/resample_oracle.py,
that statement against analytic tones (it is a definition: torchaudio is not installed, nothing recorded can stand in for
it), the WAV writer against the reader, and the file selection and refusals of cpc2_amd.eval.utils.adjust_sample_rate."""
import os
import struct

import numpy as np
import pytest
import torch

import resample_oracle as RO
from cpc2_amd import audio
from cpc2_amd.eval.utils import adjust_sample_rate as asr

PLANS = {(44100, 16000): (441, 160, 17, 475), (48000, 16000): (3, 1, 19, 41), (32000, 16000): (2, 1, 13, 28),
         (8000, 16000): (1, 2, 7, 15), (22050, 16000): (441, 320, 9, 459)}


@pytest.mark.parametrize("rates", sorted(PLANS) + [(16000, 44100)])
def test_plan_and_table_follow_the_definition(rates):
    o, n, w, taps = audio.resample_plan(*rates)
    if rates in PLANS:
        assert (o, n, w, taps) == PLANS[rates]
    else:
        assert (o, n, taps) == (160, 441, 174)
    assert (o, n, w, taps) == RO.plan(*rates)
    table = audio.resample_table(*rates)
    assert table.dtype == torch.float32 and tuple(table.shape) == (n, taps)
    assert np.array_equal(table.numpy(), RO.table(*rates).astype(np.float32))         # computed in double, rounded once


def test_plan_takes_width_and_rolloff_and_refuses_nonsense():
    assert audio.resample_plan(48000, 16000, 16, 0.945) == RO.plan(48000, 16000, 16, 0.945)
    assert np.array_equal(audio.resample_table(8000, 16000, 16, 0.945).numpy(), RO.table(8000, 16000, 16, 0.945).astype(np.float32))
    with pytest.raises(ValueError, match="orig_freq=0"):
        audio.resample_plan(0, 16000)
    with pytest.raises(ValueError, match="larger common divisor"):
        audio.resample_table(44101, 16000)


@pytest.mark.parametrize("rates", sorted(PLANS))
def test_output_length(rates):
    o, n, w, taps = RO.plan(*rates)
    for length in (0, 1, o - 1, o, o + 1):
        want = -(-n * length // o)
        assert audio.output_length(length, o, n) == want
        assert RO.resample(np.ones(length), *rates).shape == (want,)


@pytest.mark.parametrize("orig,new,freq", [(44100, 16000, 1000.0), (48000, 16000, 3000.0), (8000, 16000, 1500.0)])
def test_definition_reproduces_a_tone(orig, new, freq):
    """The fp64 statement itself: a quarter second of sin(2 pi f t + 0.3) comes out as the same tone on the new grid, within 2e-3
    away from the ends (measured 4.0e-4, 5.1e-4 and 1.2e-3: the ripple of a 6-zero-crossing Hann-windowed sinc)."""
    x = np.sin(2 * np.pi * freq * np.arange(int(orig * 0.25)) / orig + 0.3)
    y = RO.resample(x, orig, new)
    ref = np.sin(2 * np.pi * freq * np.arange(y.size) / new + 0.3)
    err = float(np.abs(y - ref)[200:-200].max())
    print(f"{orig} -> {new}, {freq} Hz: {err:.2e}")
    assert y.size > 1000 and err <= 2e-3


def test_definition_removes_a_tone_above_the_new_nyquist():
    x = np.sin(2 * np.pi * 12000.0 * np.arange(11025) / 44100 + 0.3)
    y = RO.resample(x, 44100, 16000)
    leak = float(np.abs(y)[200:-200].max())
    print(f"12 kHz through 44.1 -> 16 kHz: {leak:.2e}")
    assert y.size == 4000 and leak < 5e-3


# ----------------------------------------------------------------------------- the WAV writer
def test_write_wav_round_trip_pcm16(tmp_path):
    q = torch.tensor([[0, 1, -1, 32767, -32768, 1234], [5, -5, 100, -100, 7, 0]], dtype=torch.int16)
    path = str(tmp_path / "a.wav")
    audio.write_wav(path, q, 8000)
    raw = open(path, "rb").read()
    assert raw[:4] == b"RIFF" and raw[8:16] == b"WAVEfmt " and struct.unpack_from("<I", raw, 4)[0] == len(raw) - 8
    assert struct.unpack_from("<IHHIIHH", raw, 16) == (16, 1, 2, 8000, 8000 * 4, 4, 16)
    assert raw[36:40] == b"data" and struct.unpack_from("<I", raw, 40)[0] == 2 * 6 * 2 and len(raw) == 44 + 24
    assert audio.info(path) == (8000, 2, 6)
    wav, rate = audio.load(path)
    assert rate == 8000 and wav.dtype == torch.float32
    assert torch.equal(wav, q.float() / 32768.0)                       # channel 0 first: the order is kept


def test_save_wav_float_round_trip_on_the_host(tmp_path):
    x = torch.tensor([[0.25, -1.5, 3e-9], [1.0, 0.0, -0.125]])
    path = str(tmp_path / "f.wav")
    assert audio.save_wav(path, x, 44100, precision=32) == 0
    raw = open(path, "rb").read()
    assert struct.unpack_from("<IHHIIHH", raw, 16) == (16, 3, 2, 44100, 44100 * 8, 8, 32)
    wav, rate = audio.load(path)
    assert rate == 44100 and torch.equal(wav, x)                       # float samples are not clamped
    with pytest.raises(ValueError, match="precision=24"):
        audio.save_wav(path, x, 44100, precision=24)
    with pytest.raises(ValueError, match="channels, samples"):
        audio.save_wav(path, x[0], 44100)


def test_no_cpu_fallback(tmp_path):
    x = torch.zeros(2, 100)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        audio.resample(x, 48000, 16000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        audio.resample_pack([x[0], x[1]], 48000, 16000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        audio.save_wav(str(tmp_path / "x.wav"), x, 16000)              # PCM16 is quantised on the device
    assert not os.listdir(tmp_path)


# ----------------------------------------------------------------------------- the tool's host side
def _touch(directory, names):
    os.makedirs(directory, exist_ok=True)
    for name in names:
        path = os.path.join(directory, name)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        open(path, "wb").close()


def test_get_names_list_and_selection(tmp_path):
    phones = tmp_path / "phones.txt"
    phones.write_text("b 1 2 3\nzz 4\n\nd 5 5\n")
    assert asr.get_names_list(str(phones)) == ["b", "zz", "d"]
    db = str(tmp_path / "db")
    _touch(db, ["d.wav", "a.wav", "b.wav", "c.flac", "e.wav", "b.txt", "sub/zz.wav"])
    listed = asr.list_files(db, ".wav")
    assert sorted(listed) == ["a.wav", "b.wav", "d.wav", "e.wav"]                           # flat, by suffix
    assert sorted(asr.list_files(db, ".wav", recursive=True)) == ["a.wav", "b.wav", "d.wav", "e.wav", os.path.join("sub", "zz.wav")]
    assert asr.select_files(listed, ["b", "zz", "d"]) == ["b.wav", "d.wav"]
    assert asr.select_files(listed, None) == ["a.wav", "b.wav", "d.wav", "e.wav"]
    # a phone list that ends before the directory does: the merge ends there (the reference indexes past the end)
    assert asr.select_files(listed, ["a", "b"]) == ["a.wav", "b.wav"]
    assert asr.select_files(listed, ["0"]) == []
    assert asr.select_files(listed, []) == []
    assert asr.select_files(asr.list_files(db, ".wav", recursive=True), ["zz"]) == [os.path.join("sub", "zz.wav")]


def test_selection_follows_the_stems_not_the_paths(tmp_path):
    """The merge compares stems: neither a directory in front of a name nor the suffix behind it follows their order."""
    x, y = os.path.join("x", "b.wav"), os.path.join("y", "a.wav")
    assert asr.select_files([x, y], ["a", "b"]) == [y, x]
    tree = [os.path.join("spk1", "utt2.wav"), os.path.join("spk2", "utt1.wav"), os.path.join("spk3", "utt3.wav")]
    assert sorted(asr.select_files(tree, ["utt1", "utt2", "utt3"])) == tree
    assert asr.select_files(tree, ["utt3", "utt1"]) == [tree[1], tree[2]]
    assert asr.select_files(["a-1.wav", "a.wav", "b.wav"], ["a", "a-1"]) == ["a.wav", "a-1.wav"]     # "a-1.wav" < "a.wav", "a" < "a-1"
    same = [os.path.join("p", "u.wav"), os.path.join("q", "u.wav"), os.path.join("q", "v.wav")]
    assert asr.select_files(same, ["u"]) == same[:2]                                   # files that share a stem are all taken
    assert asr.select_files([x, y], None) == [y, x]
    db = str(tmp_path / "db")
    _touch(db, ["x/b.wav", "y/a.wav", "y/c.WAV", "y/c.flac"])
    listed = asr.list_files(db, ".wav", recursive=True)
    assert asr.select_files(listed, ["c", "b", "a"]) == [y, x, os.path.join("y", "c.WAV")]     # the suffix: without regard to case
    assert sorted(asr.list_files(db, ".WAV", recursive=True)) == sorted(listed)
    assert asr.list_files(os.path.join(db, "y"), ".Wav") and len(asr.list_files(os.path.join(db, "y"), ".Wav")) == 2


def test_without_a_device_the_tool_refuses_before_it_creates_anything(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    db, out = str(tmp_path / "db"), str(tmp_path / "out")
    _touch(db, ["a.wav"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        asr.main([db, out])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        asr.adjust_sample_rate(db, ["a.wav"], out, 16000)
    assert not os.path.exists(out)


def test_two_inputs_of_one_output_are_refused(tmp_path, monkeypatch):
    monkeypatch.setattr(asr, "require_device", lambda: torch.device("cpu"))           # (the check comes before any device work)
    db, out = str(tmp_path / "db"), str(tmp_path / "out")
    _touch(db, ["a.wav", "a.WAV"])
    if len(os.listdir(db)) == 2:                                                       # (a file system that tells the two apart)
        with pytest.raises(ValueError, match="would both be written"):
            asr.main([db, out])
        assert not os.path.exists(out)


def test_command_line_arguments():
    args = asr.parse_args(["db", "phones.txt", "out"])
    assert (args.path_db, args.path_phone_files, args.path_out) == ("db", "phones.txt", "out")
    assert args.out_sample_rate == 16000 and args.file_extension == ".wav" and not args.recursive
    args = asr.parse_args(["db", "out", "--out_sample_rate", "8000", "--file_extension", ".flac", "--recursive"])
    assert (args.path_db, args.path_phone_files, args.path_out) == ("db", None, "out")
    assert args.out_sample_rate == 8000 and args.file_extension == ".flac" and args.recursive
    assert all(callable(getattr(asr, name)) for name in ("adjust_sample_rate", "get_names_list", "parse_args", "main"))


def test_mp3_and_a_non_empty_output_are_refused_before_anything_is_read(tmp_path):
    db, out = str(tmp_path / "db"), str(tmp_path / "out")
    _touch(db, ["a.mp3", "a.wav"])                                       # (empty files: reading one would fail differently)
    with pytest.raises(ValueError, match=r"--file_extension \.mp3.*no mp3 decoder"):
        asr.main([db, out, "--file_extension", ".mp3"])
    with pytest.raises(ValueError, match=r"--file_extension \.ogg.*\.wav and \.flac"):
        asr.main([db, out, "--file_extension", ".ogg"])
    assert not os.path.exists(out)
    _touch(out, ["keep.me"])
    with pytest.raises(ValueError, match="path_out .* exists and is not empty"):
        asr.main([db, out])
    assert os.listdir(out) == ["keep.me"]
