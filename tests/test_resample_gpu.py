"""Sample-rate conversion on the GPU (csrc/resample.hip through cpc2_amd.audio): unit impulses against the f32 table bit for
bit, random signals against the fp64 statement of tests/resample_oracle.py within the first-order bound of an f32 dot product,
packs against single signals bit for bit with canaries around every segment, the PCM16 quantiser, and the
adjust_sample_rate tool end to end on the FLAC fixtures."""
import os

import numpy as np
import pytest
import torch

import resample_oracle as RO
from cpc2_amd import audio
from cpc2_amd.eval.utils import adjust_sample_rate as asr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DB = os.path.join(ROOT, "tests", "golden", "test_db")
DEV = "cuda:0"
RATES = [(48000, 16000), (32000, 16000), (8000, 16000), (44100, 16000), (16000, 44100)]
CANARY = 1e30


def _lengths(o):
    return sorted({1, o - 1, o, o + 1, 16 * o + 1} - {0})


@pytest.fixture(scope="module")
def tables():
    """rates -> (plan, f32 table as the library makes it, fp64 table of the oracle); made once, never written."""
    made = {}
    for rates in RATES + [(22050, 16000)]:
        t32, t64 = audio.resample_table(*rates).numpy(), RO.table(*rates)
        t32.setflags(write=False)
        t64.setflags(write=False)
        made[rates] = (RO.plan(*rates), t32, t64)
    return made


@pytest.mark.parametrize("rates", RATES)
def test_unit_impulse_returns_the_table_bit_for_bit(tables, rates):
    """x = delta at i: output f n + p is h[p][i + w - f o] where that index is inside the table and 0 elsewhere -- a sum of one
    table entry and zeros is exact, so equality holds without a tolerance."""
    (o, n, w, taps), h, _h64 = tables[rates]
    for length in _lengths(o):
        at = sorted({0, length - 1, length // 2})
        x = torch.zeros(len(at), length)
        for row, i in enumerate(at):
            x[row, i] = 1.0
        y = audio.resample(x.to(DEV), *rates).cpu().numpy()
        out_len = -(-n * length // o)
        assert y.shape == (len(at), out_len)
        m = np.arange(out_len)
        f, p = m // n, m % n
        for row, i in enumerate(at):
            j = i + w - f * o
            inside = (j >= 0) & (j < taps)
            want = np.where(inside, h[p, np.clip(j, 0, taps - 1)], np.float32(0.0))
            assert inside.any()
            assert np.array_equal(y[row], want), (rates, length, i, int((y[row] != want).sum()))


# ratios at which the library takes another path than the rate pairs above do: one and two phases per lane of the many-phase
# kernel (n = 64, 128; the pairs above take three and four), fewer frames per workgroup than threads could hold because the
# signal segment fills the LDS array (o = 1001) in both kernels, and phase lanes without a phase (n = 3 of 4, n = 48 of 64)
OTHER_PATHS = [(3, 64), (5, 128), (1001, 64), (1001, 8), (32000, 48000), (7, 48)]


@pytest.mark.parametrize("rates", OTHER_PATHS)
def test_every_kernel_path_against_the_definition(rates):
    o, n, w, taps = RO.plan(*rates)
    h, h64 = audio.resample_table(*rates).numpy(), RO.table(*rates)
    g = torch.Generator().manual_seed(o + n)
    for length in (o + 1, 16 * o + 1) if o < 1000 else (o + 1, 7 * o + 1):
        x = 0.3 * torch.randn(length, generator=g)
        x[length // 2] = 0.0
        impulse = torch.zeros(length)
        impulse[length // 2] = 1.0
        y = audio.resample(torch.stack([x, impulse]).to(DEV), *rates).cpu().numpy()
        y64, scale = RO.resample(x.numpy(), *rates, h=h64, with_bound_sum=True)
        bound = (taps + 4) * 2.0 ** -24 * scale + taps * 2.0 ** -126
        assert y.shape == (2, y64.size) and float((np.abs(y[0] - y64) / bound).max()) <= 1.0, (rates, length)
        m = np.arange(y64.size)
        j = length // 2 + w - (m // n) * o
        want = np.where((j >= 0) & (j < taps), h[m % n, np.clip(j, 0, taps - 1)], np.float32(0.0))
        assert np.array_equal(y[1], want), (rates, length)


def test_a_ratio_too_irregular_for_a_workgroup_is_refused_by_name():
    with pytest.raises(ValueError, match=r"reduced ratio o / n = 5000 / 3 .* larger common divisor"):
        audio.resample(torch.zeros(100, device=DEV), 5000, 3)


@pytest.mark.parametrize("rates", RATES + [(22050, 16000)])
def test_random_signals_within_the_f32_dot_product_bound(tables, rates):
    """|y - y64| <= (taps + 4) 2^-24 sum_j |h64[p][j]| |xp[j]| + taps 2^-126 per output sample: the first-order bound of an f32 dot
    product of `taps` terms in any order with a table rounded once, plus the products that underflow (the window's last taps are
    about 1e-49).  Two f32 summation orders on the CPU stay below 0.11 of it."""
    (o, n, w, taps), _h, h64 = tables[rates]
    g = torch.Generator().manual_seed(1000 + o + n)
    worst = 0.0
    for length in _lengths(o):
        x = 0.3 * torch.randn(length, generator=g)
        y = audio.resample(x.to(DEV), *rates).double().cpu().numpy()
        y64, scale = RO.resample(x.numpy(), *rates, h=h64, with_bound_sum=True)
        assert y.shape == y64.shape and np.isfinite(y).all()
        bound = (taps + 4) * 2.0 ** -24 * scale + taps * 2.0 ** -126
        ratio = float((np.abs(y - y64) / bound).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (rates, length, ratio)
    print(f"{rates}: worst |y - y64| / bound = {worst:.3f}")


@pytest.mark.parametrize("rates", RATES)
def test_pack_equals_single_signals_and_keeps_its_segments(tables, rates):
    (o, n, w, taps), _h, _h64 = tables[rates]
    lengths = [1, 7, o, 3 * o + 5, 16 * o + 1]
    g = torch.Generator().manual_seed(7)
    signals = [0.3 * torch.randn(v, generator=g) for v in lengths]
    single = [audio.resample(s.to(DEV), *rates).cpu() for s in signals]
    results = []
    for order in ([0, 1, 2, 3, 4], [4, 2, 0, 3, 1]):
        flat, offsets, at = [], [], 0
        for k in order:                                   # 1e30 in front of, between and behind the signals
            flat.append(torch.full((3 + k,), CANARY))
            at += 3 + k
            offsets.append(at)
            flat.append(signals[k])
            at += lengths[k]
        flat.append(torch.full((5,), CANARY))
        out_lens = [-(-n * lengths[k] // o) for k in order]
        out_offsets = [0] * 5
        for i in range(1, 5):
            out_offsets[i] = out_offsets[i - 1] + out_lens[i - 1] + 2
        out = torch.full((out_offsets[-1] + out_lens[-1] + 2,), CANARY, device=DEV)
        views = audio.resample_pack(torch.cat(flat).to(DEV), *rates, lengths=[lengths[k] for k in order], offsets=offsets,
                                    out=out, out_offsets=out_offsets)
        host = out.cpu()
        for i, k in enumerate(order):
            assert views[i].data_ptr() == out.data_ptr() + 4 * out_offsets[i] and views[i].numel() == out_lens[i]
            assert torch.equal(views[i].cpu(), single[k]), (rates, order, k)           # bitwise: no neighbour, no tiling shows
            assert torch.all(host[out_offsets[i] + out_lens[i]:out_offsets[i] + out_lens[i] + 2] == CANARY), (rates, order, k)
        results.append({k: views[i].cpu() for i, k in enumerate(order)})
    assert all(torch.equal(results[0][k], results[1][k]) for k in range(5))
    listed = audio.resample_pack([s.to(DEV) for s in signals], *rates)                  # the list form: a dense output
    assert all(torch.equal(a.cpu(), b) for a, b in zip(listed, single))
    assert listed[1].data_ptr() == listed[0].data_ptr() + 4 * listed[0].numel()


def test_pcm16_quantiser_and_its_clamp_count():
    g = torch.Generator().manual_seed(3)
    x = 0.3 * torch.randn(7057, generator=g)
    y = audio.resample(x.to(DEV), 44100, 16000)
    ties = torch.tensor([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 32767.5, -32768.5, 32767.0, -32768.0, 32768.0, -32769.0]) / 32768.0
    for scale, extra in ((1.0, ties), (4.0, ties)):
        v = torch.cat([y * scale, extra.to(DEV)])
        q, clamped = audio.to_pcm16(v)
        r = np.rint(v.cpu().numpy() * np.float32(32768.0))
        want = np.clip(r, -32768, 32767).astype(np.int16)
        assert q.dtype == torch.int16 and np.array_equal(q.cpu().numpy(), want)
        count = int(((r < -32768) | (r > 32767)).sum())
        assert int(clamped.item()) == count
        assert (count > 100) == (scale == 4.0) and count >= 3          # (32768 and -32769 and 32767.5 -> 32768 are clamped)
    assert q.cpu().numpy()[-12:-6].tolist() == [0, 2, 2, 0, -2, -2]    # ties to even


def test_save_wav_pcm16_reads_back(tmp_path):
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 3001, generator=g) * 0.5
    path = str(tmp_path / "s.wav")
    clamped = audio.save_wav(path, x.to(DEV), 22050)
    r = np.rint(x.numpy() * np.float32(32768.0))
    assert clamped == int(((r < -32768) | (r > 32767)).sum()) and clamped > 0
    wav, rate = audio.load(path)
    assert rate == 22050 and audio.info(path) == (22050, 2, 3001)
    assert np.array_equal(wav.numpy(), np.clip(r, -32768, 32767).astype(np.float32) / np.float32(32768.0))
    assert audio.save_wav(path, x.to(DEV), 22050, precision=32) == 0
    assert torch.equal(audio.load(path)[0], x)


def test_device_tables_are_cached_within_a_bound(monkeypatch):
    audio._tables.clear()
    x = torch.zeros(64, device=DEV)
    audio.resample(x, 48000, 16000)
    first = next(iter(audio._tables.values()))
    audio.resample(x, 48000, 16000)
    assert len(audio._tables) == 1 and next(iter(audio._tables.values())) is first       # reused, not rebuilt
    for new in range(2, 2 + audio.MAX_CACHED_TABLES):
        audio.resample(x, 1, new)
    assert len(audio._tables) == audio.MAX_CACHED_TABLES and all(t is not first for t in audio._tables.values())
    monkeypatch.setattr(audio, "MAX_CACHED_FLOATS", 100)                 # the tables beside the one in use: at most 100 floats
    audio.resample(x, 44100, 16000)
    assert sum(t.numel() for t in list(audio._tables.values())[:-1]) <= 100 and list(audio._tables.values())[-1].numel() == 160 * 475


def test_equal_rates_return_the_input_without_a_launch(monkeypatch):
    def no_launch(*_a, **_k):
        raise AssertionError("a kernel was launched for equal rates")
    monkeypatch.setattr(audio, "_launch", no_launch)
    x = torch.randn(2, 100, device=DEV)
    assert audio.resample(x, 16000, 16000) is x
    views = audio.resample_pack(x.view(-1), 44100, 44100, lengths=[100, 100])
    assert [v.data_ptr() for v in views] == [x.data_ptr(), x.data_ptr() + 400] and torch.equal(views[1], x[1])


@pytest.mark.parametrize("rates", [(44100, 16000), (48000, 16000), (8000, 16000)])
def test_channels_are_resampled_independently(rates):
    g = torch.Generator().manual_seed(5)
    x = (0.3 * torch.randn(2, 3, 1501, generator=g)).to(DEV)
    y = audio.resample(x, *rates)
    o, n, _w, _taps = RO.plan(*rates)
    assert y.shape == (2, 3, -(-n * 1501 // o))
    for a in range(2):
        for b in range(3):
            assert torch.equal(y[a, b], audio.resample(x[a, b], *rates))
    strided = x[:, :, ::2]                                              # a non-contiguous input is taken as its values
    assert torch.equal(audio.resample(strided, *rates), audio.resample(strided.contiguous(), *rates))


def test_tool_end_to_end_on_the_flac_fixtures(tmp_path, capsys):
    names = ["2911-12359-0007", "4051-11218-0044", "4397-15668-0003"]
    rel = {"2911-12359-0007": "2911/12359", "4051-11218-0044": "4051/11218", "4397-15668-0003": "4397/15668"}
    phones = tmp_path / "phones.txt"
    phones.write_text("".join(f"{name} 1 2 3\n" for name in names))
    out8, out16 = str(tmp_path / "at8k"), str(tmp_path / "at16k")
    clamped = asr.main([DB, str(phones), out8, "--out_sample_rate", "8000", "--file_extension", ".flac", "--recursive"])
    printed = capsys.readouterr().out
    assert "Converting 3 files" in printed and f"Clamped {clamped} samples" in printed
    asr.main([out8, out16, "--recursive"])
    assert "Converting 3 files" in capsys.readouterr().out
    total = 0
    for name in names:
        src, rate = audio.load(os.path.join(DB, rel[name], name + ".flac"))
        assert rate == 16000
        p8, p16 = os.path.join(out8, rel[name], name + ".wav"), os.path.join(out16, rel[name], name + ".wav")
        length = src.shape[1]
        assert audio.info(p8) == (8000, 1, -(-length // 2))
        assert audio.info(p16) == (16000, 1, 2 * -(-length // 2))
        q, c = audio.to_pcm16(audio.resample(src.to(DEV), 16000, 8000))
        total += int(c.item())
        assert torch.equal(audio.load(p8)[0], q.cpu().float() / 32768.0)                # the file is resample + quantisation
    assert total == clamped
    assert sorted(os.listdir(out8)) == ["2911", "4051", "4397"]
