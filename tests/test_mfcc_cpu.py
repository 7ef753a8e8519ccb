"""cpc2_amd.spectral without a GPU: the oracle (tests/mfcc_oracle.py) against independent pieces, the library's host tables
against the oracle's, the new symbols, every refusal of the C entry points before any launch, and the command line of
build_baseline_features with its refusals before the directory is listed."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.fft
import scipy.signal
import torch

import mfcc_oracle as O
from cpc2_amd import _lib
from cpc2_amd import dataset as ds
from cpc2_amd import spectral
from cpc2_amd.eval import build_baseline_features as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("cpc_mfcc_tables_doubles", "cpc_mfcc_tables_host", "cpc_mfcc_frame_tile", "cpc_melspec_scratch_bytes",
               "cpc_melspec_db", "cpc_mfcc_finish", "cpc_deltas")


# --------------------------------------------------------------------------- the oracle against independent pieces
@pytest.mark.parametrize("n_out,n_mels", [(13, 40), (40, 40), (64, 128), (1, 1), (128, 128)])
def test_oracle_dct_is_scipys_orthonormal_dct2(n_out, n_mels):
    """The definition's cos(pi / n_mels (m + 0.5) k) has an argument of up to pi n_out, whose own rounding (pi n_out 2^-53) times
    sqrt(2 / n_mels) stays below 1e-14 up to n_out = 128; at 512 x 512 the formula as written is 1.1e-14 from the exact matrix."""
    ref = scipy.fft.dct(np.eye(n_mels), type=2, norm="ortho", axis=0)          # column m = the DCT of unit vector m
    assert np.abs(O.dct_matrix(n_out, n_mels) - ref[:n_out]).max() <= 1e-14


@pytest.mark.parametrize("n", [32, 64, 321, 400, 512])
def test_oracle_window_is_scipys_periodic_hann(n):
    assert np.abs(O.window(n) - scipy.signal.get_window("hann", n, fftbins=True)).max() <= 1e-15


def _reflect_by_hand(i, L):
    if i < 0:
        return -i
    if i >= L:
        return 2 * (L - 1) - i
    return i


@pytest.mark.parametrize("grid", ["cpc", "center"])
@pytest.mark.parametrize("L", [161, 320, 321, 481])
def test_oracle_frames_of_a_ramp_are_the_reflected_indices(L, grid):
    n_fft, hop = 321, 160
    offset, frames_of = O.grid_of(grid, hop)
    T = frames_of(L)
    assert T == (L // 160 if grid == "cpc" else 1 + L // 160) and offset == (80 if grid == "cpc" else 0)
    idx = O.frame_indices(L, n_fft, hop, offset, T)
    assert idx.shape == (T, n_fft)
    for t in range(T):
        centre = t * hop + offset
        want = [_reflect_by_hand(centre - 160 + n, L) for n in range(n_fft)]
        assert idx[t].tolist() == want, (t, grid)
        assert idx[t, 160] == centre if centre < L else idx[t, 160] == 2 * (L - 1) - centre
    # a ramp read through them is the indices themselves: the frames of the signal x[i] = i
    ramp = np.arange(L, dtype=np.float32)
    assert np.array_equal(ramp[idx], idx.astype(np.float32))
    # spelled out for the shortest signal: 161 samples, frame 0 of the centred grid reads 160 .. 1, 0, 1 .. 160
    if L == 161 and grid == "center":
        assert idx[0].tolist() == list(range(160, 0, -1)) + list(range(0, 161))
        assert idx[1].tolist() == list(range(0, 161)) + list(range(159, -1, -1))
    if L == 161 and grid == "cpc":
        assert idx[0].tolist() == list(range(80, 0, -1)) + list(range(0, 161)) + list(range(159, 79, -1))
    with pytest.raises(ValueError):
        O.frame_indices(160, n_fft, hop, offset, 1)


def test_oracle_power_of_an_impulse_is_the_window_squared():
    n_fft, hop, L = 321, 160, 481
    fb = np.eye(n_fft // 2 + 1)                                   # "filterbank" that returns the power spectrum itself
    for p in (0, 100, 240, 480):
        x = np.zeros(L, dtype=np.float32)
        x[p] = 1.0
        P, _ = O.linear_mel(x, n_fft, hop, 80, L // hop, fb)
        idx = O.frame_indices(L, n_fft, hop, 80, L // hop)
        for t in range(L // hop):
            hits = np.flatnonzero(idx[t] == p)
            if len(hits) == 1:
                assert np.abs(P[t] - O.window(n_fft)[hits[0]] ** 2).max() <= 1e-14


# --------------------------------------------------------------------------- the library's tables
def _sections(t, n_fft, n_mels, n_out):
    Wp, F = (n_fft + 3) // 4 * 4, n_fft // 2 + 1               # the twiddles' rows n <= n_fft // 2: the kernel folds n_fft - n onto n
    Hp, Fp, Mp = (F + 3) // 4 * 4, (F + 15) // 16 * 16, (n_mels + 15) // 16 * 16
    assert t.size == Wp + 2 * Hp * Fp + Fp * Mp + n_mels * n_out
    o = 0
    win = t[o:o + Wp]
    o += Wp
    cos = t[o:o + Hp * Fp].reshape(Hp, Fp)
    o += Hp * Fp
    sin = t[o:o + Hp * Fp].reshape(Hp, Fp)
    o += Hp * Fp
    fb = t[o:o + Fp * Mp].reshape(Fp, Mp)
    o += Fp * Mp
    return win, cos, sin, fb, t[o:].reshape(n_mels, n_out)


def _within_2_ulp(got, ref):
    return bool(np.all(np.abs(got - ref) <= 2.0 * np.spacing(np.maximum(np.abs(got), np.abs(ref)))))


@pytest.mark.parametrize("n_fft,n_mels,n_out", [(321, 128, 64), (400, 40, 13), (64, 40, 13)])
def test_host_tables_are_the_oracles(n_fft, n_mels, n_out):
    t = spectral.host_tables(n_fft, n_mels, n_out).numpy()
    win, cos, sin, fb, dctT = _sections(t, n_fft, n_mels, n_out)
    F = n_fft // 2 + 1
    ref_cos, ref_sin = O.twiddles(n_fft)
    ref_fb = O.mel_filterbank(n_fft, n_mels)
    assert _within_2_ulp(win[:n_fft], O.window(n_fft))
    assert _within_2_ulp(cos[:F, :F], ref_cos[:F]) and _within_2_ulp(sin[:F, :F], ref_sin[:F])
    # the rows that are not stored are those rows mirrored: cos even, sin odd about n_fft / 2
    assert np.abs(ref_cos[1:][::-1][:F - 1] - ref_cos[1:F]).max() <= 1e-13 and np.abs(ref_sin[1:][::-1][:F - 1] + ref_sin[1:F]).max() <= 1e-13
    assert _within_2_ulp(fb[:F, :n_mels], ref_fb)
    assert _within_2_ulp(dctT.T, O.dct_matrix(n_out, n_mels))
    # the padding the kernels read is zero, and so are the filters that catch no bin (n_mels = 128 over 161 bins: 8 of them)
    assert not win[n_fft:].any() and not cos[F:].any() and not sin[F:].any()
    assert not cos[:, F:].any() and not sin[:, F:].any() and not fb[F:].any() and not fb[:, n_mels:].any()
    empty = np.flatnonzero(ref_fb.sum(axis=0) == 0.0)
    assert len(empty) == {(321, 128): 8, (400, 40): 0, (64, 40): 7}[(n_fft, n_mels)]
    assert not fb[:, empty].any() and np.array_equal(np.flatnonzero(fb[:F, :n_mels].sum(axis=0) == 0.0), empty)


# --------------------------------------------------------------------------- the C entry points
def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "cpc2_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in cpc2_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES
    assert _lib.load().cpc_version() >= 119
    assert _lib.load().cpc_mfcc_frame_tile() == spectral.FRAME_TILE


def test_entry_points_refuse_by_name_before_any_launch():
    lib = _lib.load()
    one = ctypes.c_void_p(256)                                          # never dereferenced: refused before any launch

    def err():
        return lib.cpc_last_error().decode()

    # ---- tables
    assert lib.cpc_mfcc_tables_doubles(321, 128, 64) == 324 + 2 * 164 * 176 + 176 * 128 + 128 * 64
    for bad in [(31, 40, 13), (513, 40, 13), (400, 0, 1), (400, 513, 13), (400, 40, 0), (400, 40, 41)]:
        assert lib.cpc_mfcc_tables_doubles(*bad) == 0 and "mfcc_tables_doubles: parameters outside" in err()
        assert lib.cpc_mfcc_tables_host(*bad, 16000, 0.0, 8000.0, one, 1 << 40) == -1 and "mfcc_tables_host: parameters outside" in err()
    assert lib.cpc_mfcc_tables_host(400, 40, 13, 1, 0.0, 8000.0, one, 1 << 40) == -1 and "sample_rate=1" in err()
    assert lib.cpc_mfcc_tables_host(400, 40, 13, 16000, 8000.0, 8000.0, one, 1 << 40) == -1 and "f_min < f_max" in err()
    assert lib.cpc_mfcc_tables_host(400, 40, 13, 16000, 0.0, 8000.0, one, 10) == -1 and "room for 10 doubles" in err()
    assert lib.cpc_mfcc_tables_host(400, 40, 13, 16000, 0.0, 8000.0, None, 1 << 40) == -1

    # ---- scratch query
    assert lib.cpc_melspec_scratch_bytes(3, 2, 40) >= 8 * (3 * 16 * 40 + 3 + 2)
    for bad in [(0, 1, 40), (3, 0, 40), (3, 2, 0), (3, 2, 513), (1 << 31, 1, 40)]:
        assert lib.cpc_melspec_scratch_bytes(*bad) == 0 and "melspec_scratch_bytes" in err()

    # ---- melspec_db
    def db(n_fft=400, hop=160, offset=80, n_mels=40, count=1, tiles=1, min_len=400, floor_mode=1, top_db=80.0, x=one, tables=one,
           scratch=one, nbytes=1 << 40):
        return lib.cpc_melspec_db(x, 1000, one, one, one, one, count, tiles, min_len, n_fft, hop, offset, n_mels, tables, floor_mode,
                                  top_db, scratch, nbytes, None)
    for kw, text in [(dict(n_fft=31), "n_fft=31 outside 32..512"), (dict(n_fft=513), "n_fft=513 outside 32..512"),
                     (dict(hop=0), "hop=0 outside 1..n_fft"), (dict(hop=401), "hop=401 outside 1..n_fft"),
                     (dict(offset=-1), "offset=-1 outside 0..hop"), (dict(offset=161), "offset=161 outside 0..hop"),
                     (dict(n_mels=0), "n_mels=0 outside 1..512"), (dict(n_mels=513), "n_mels=513 outside 1..512"),
                     (dict(count=0), "count=0"), (dict(tiles=0), "total_tiles=0"),
                     (dict(min_len=200), "a signal of 200 samples is too short"),
                     (dict(n_fft=321, min_len=160), "a signal of 160 samples is too short"),
                     (dict(floor_mode=3), "floor_mode=3"), (dict(top_db=-1.0), "top_db=-1"),
                     (dict(top_db=float("nan")), "top_db=nan"), (dict(x=None), "null buffer"), (dict(tables=None), "null buffer"),
                     (dict(scratch=None), "scratch of"), (dict(nbytes=16), "scratch of 16 bytes")]:
        assert db(**kw) == -1 and "melspec_db: " + text in err(), (kw, err())

    # ---- mfcc_finish
    def finish(n_fft=400, n_mels=40, n_out=13, want_dct=1, count=1, tiles=1, floor_mode=1, ldo=13, out_rows=16, out=one, tables=one,
               scratch=one, nbytes=1 << 40):
        return lib.cpc_mfcc_finish(scratch, nbytes, one, one, one, count, tiles, n_fft, n_mels, n_out, want_dct, tables, floor_mode,
                                   out, ldo, out_rows, None)
    for kw, text in [(dict(n_fft=16), "n_fft=16 outside 32..512"), (dict(n_mels=600), "n_mels=600 outside 1..512"),
                     (dict(n_out=0), "n_out=0 outside 1..n_mels"), (dict(n_out=41), "n_out=41 outside 1..n_mels"),
                     (dict(want_dct=0), "the dB rows have n_mels=40 columns, not n_out=13"), (dict(count=0), "count=0"),
                     (dict(tiles=0), "total_tiles=0"), (dict(floor_mode=-1), "floor_mode=-1"), (dict(ldo=12), "row stride"),
                     (dict(out_rows=0), "row stride"), (dict(out=None), "null buffer"), (dict(tables=None), "null buffer"),
                     (dict(nbytes=16), "scratch of 16 bytes")]:
        assert finish(**kw) == -1 and "mfcc_finish: " + text in err(), (kw, err())

    # ---- deltas
    def deltas(cols=13, count=1, max_frames=5, ldi=13, ldo=13, rows=5, src=one, dst=one):
        return lib.cpc_deltas(src, ldi, dst, ldo, cols, one, one, count, max_frames, rows, None)
    for kw, text in [(dict(cols=0), "cols=0"), (dict(cols=1537, ldi=1537, ldo=1537), "cols=1537"), (dict(count=0), "count=0"),
                     (dict(count=65536), "count=65536"), (dict(max_frames=0), "max_frames=0"), (dict(ldi=12), "row stride"),
                     (dict(ldo=12), "row stride"), (dict(rows=0), "row stride"), (dict(src=None), "null buffer"),
                     (dict(dst=None), "null buffer")]:
        assert deltas(**kw) == -1 and "deltas: " + text in err(), (kw, err())


def test_python_objects_refuse_by_name_and_host_tensors():
    for kw, text in [(dict(n_fft=16), "n_fft=16"), (dict(n_fft=600), "n_fft=600"), (dict(hop=0), "hop=0"), (dict(hop=401), "hop=401"),
                     (dict(n_mels=0), "n_mels=0"), (dict(n_mels=513), "n_mels=513"), (dict(n_mfcc=41), "n_mfcc=41"),
                     (dict(top_db=-3.0), "top_db=-3.0"), (dict(grid="left"), "grid='left'"), (dict(floor="batch"), "floor='batch'")]:
        with pytest.raises(ValueError, match=re.escape(text)):
            spectral.MFCC(**kw)
    with pytest.raises(ValueError, match="n_mels=0"):
        spectral.MelSpectrogramDB(n_mels=0)
    m = spectral.MFCC()
    assert (m.n_frames(20480), spectral.MFCC(grid="center").n_frames(20480), m.offset) == (128, 129, 80)
    for call in (lambda: m(torch.zeros(2, 1000)), lambda: m([torch.zeros(1000)]), lambda: m(torch.zeros(1000), lengths=[1000]),
                 lambda: spectral.compute_deltas(torch.zeros(5, 13))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    r = spectral.MFCC.reference_encoder(64)
    assert (r.n_fft, r.hop, r.offset, r.n_mels, r.n_out, r.top_db, r.floor, r.grid) == (321, 160, 0, 128, 64, 80.0, "call", "center")
    assert spectral.MFCC.reference_encoder(256).n_mels == 256


def test_training_on_mfccs_stays_refused():
    import types
    from cpc2_amd.train import getEncoder
    with pytest.raises(NotImplementedError):
        getEncoder(types.SimpleNamespace(encoder_type="mfcc", hiddenEncoder=256, normMode="layerNorm"))


# --------------------------------------------------------------------------- the tool's command line
def test_parser_defaults_and_the_reference_encoder():
    args = B.parse_args(["db", "out"])
    assert vars(args) == dict(path_audio="db", path_out="out", type="mfcc", n_mfcc=13, n_mels=40, n_fft=400, hop=160, deltas=None,
                              seqNorm=False, top_db=80.0, grid="cpc", reference_encoder=None, format="pt", file_extension=".wav",
                              sample_rate=16000, pack_bytes=1 << 28, debug=False)
    params, deltas = B.feature_parameters(args)
    assert deltas == 2 and params == dict(kind="mfcc", sample_rate=16000, n_fft=400, hop=160, n_mels=40, n_mfcc=13, top_db=80.0,
                                          floor="signal", grid="cpc")
    params, deltas = B.feature_parameters(B.parse_args(["db", "out", "--type", "mel", "--top_db", "-1", "--deltas", "0"]))
    assert deltas == 0 and params["kind"] == "mel" and params["top_db"] is None and "n_mfcc" not in params
    # cpc/model.py:117-120: n_mels = max(128, dimEncoded), n_fft = 321, n_mfcc = dimEncoded (torchaudio: hop = 321 // 2, centred)
    params, deltas = B.feature_parameters(B.parse_args(["db", "out", "--reference_encoder", "256", "--n_fft", "512", "--type", "mel"]))
    assert deltas == 0 and params == dict(kind="mfcc", sample_rate=16000, n_mfcc=256, n_fft=321, hop=160, n_mels=256, top_db=80.0,
                                          floor="signal", grid="center")
    assert B.feature_parameters(B.parse_args(["db", "out", "--reference_encoder", "64"]))[0]["n_mels"] == 128
    t = B.make_transform(params)
    assert isinstance(t, spectral.MFCC) and (t.n_fft, t.n_mels, t.n_out, t.offset) == (321, 256, 256, 0)
    for bad in (["db"], ["db", "out", "--type", "lfb"], ["db", "out", "--format", "af"], ["db", "out", "--grid", "left"]):
        with pytest.raises(SystemExit):
            B.parse_args(bad)


REFUSED = [(["--file_extension", ".mp3"], NotImplementedError, r"--file_extension \.mp3: there is no mp3 decoder"),
           (["--n_fft", "16"], ValueError, "outside the kernel's domain: n_fft=16"),
           (["--n_fft", "1024"], ValueError, "outside the kernel's domain: n_fft=1024"),
           (["--hop", "401"], ValueError, "outside the kernel's domain: hop=401"),
           (["--n_mels", "600"], ValueError, "outside the kernel's domain: n_mels=600"),
           (["--n_mfcc", "41"], ValueError, "outside the kernel's domain: n_mfcc=41"),
           (["--reference_encoder", "600"], ValueError, "outside the kernel's domain: n_mels=600"),
           (["--deltas", "3"], ValueError, "--deltas 3"),
           (["--pack_bytes", "0"], ValueError, "--pack_bytes 0")]


@pytest.mark.parametrize("flags,kind,text", REFUSED, ids=[" ".join(r[0]) for r in REFUSED])
def test_main_refuses_by_name_before_the_audio_is_listed(flags, kind, text, monkeypatch, tmp_path):
    listed = []
    monkeypatch.setattr(ds, "findAllSeqs", lambda *a, **k: listed.append(a) or ([], []))
    out = tmp_path / "out"
    with pytest.raises(kind, match=text):
        B.main([str(tmp_path / "db"), str(out)] + flags)
    assert not listed and not out.exists()


def test_main_refuses_a_directory_that_is_not_empty(monkeypatch, tmp_path):
    listed = []
    monkeypatch.setattr(ds, "findAllSeqs", lambda *a, **k: listed.append(a) or ([], []))
    out = tmp_path / "out"
    out.mkdir()
    (out / "kept.pt").write_bytes(b"x")
    with pytest.raises(ValueError, match="exists and is not an empty directory"):
        B.main([str(tmp_path / "db"), str(out)])
    assert not listed and sorted(p.name for p in out.iterdir()) == ["kept.pt"]


def test_a_file_at_another_rate_is_refused_with_the_command(tmp_path):
    from cpc2_amd import audio
    path = tmp_path / "a.wav"
    audio.write_wav(str(path), np.zeros((2, 800), dtype=np.float32), 8000)
    with pytest.raises(ValueError, match=r"8000 Hz, not --sample_rate 16000.*cpc2_amd\.eval\.utils\.adjust_sample_rate .* --out_sample_rate 16000"):
        B.load_mono(str(path), 16000, str(tmp_path))
    stereo = np.stack([np.full(800, 0.5, dtype=np.float32), np.full(800, -0.25, dtype=np.float32)])
    audio.write_wav(str(path), stereo, 16000)
    mono = B.load_mono(str(path), 16000)
    assert mono.shape == (800,) and torch.equal(mono, torch.full((800,), 0.125))
