"""The `bandreject_sinc` kernels (csrc/bandreject.hip) against the numpy statement of tests/bandreject_oracle.py.

The design on its own: every tap within 2^-40 of the statement's (libm is a few ulp and the sine's argument, |j| <= 1024, is held
to 2^-41).  Exact properties by equality: an impulse comes back as the rounded taps wherever it sits (halo, fold and tile seams),
identity rows bit for bit, zero in / zero out, and what the definition promises about packs, batches, launches and overhang.
Accuracy for every sample: |y - y64| <= 2^-24 |y64| + 2^-38 sum_j |x[t - j]| + 2^-149 -- one f32 rounding, a tap error of 2^-40
and at most 2049 f64 roundings, a factor 2 of margin.  Then the transform, the direct call, the feeder and the command line.

No case has more than 8 rows or more than 3 tile + 5 samples, tile from cpc_bandreject_tile()."""
import functools
import json
import os
import random

import numpy as np
import pytest
import torch

import bandreject_oracle as BO
from cpc2_amd import _lib
from cpc2_amd import audio
from cpc2_amd import data_augmentation as da
from cpc2_amd import dataset as ds
from cpc2_amd import train as tr
from cpc2_amd._lib import ptr, stream_ptr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DB = os.path.join(ROOT, "tests", "golden", "test_db")
SEQ_LIST = os.path.join(ROOT, "tests", "golden", "seq_list.txt")
with open(os.path.join(ROOT, "tests", "golden", "g30_bandreject_draws.json")) as _fh:
    GOLDEN = json.load(_fh)
DEV = "cuda:0"
SR = 16000.0
BETA = BO.design()[0]
BANDS = [(0.0, 0.0), (0.0, 500.0), (1000.0, 2000.0), (7000.0, 8000.0), (3000.0, 3010.0), (0.0, 8000.0), (0.12, 7999.5)]
HALVES = [1, 2, 157, 1024]
NAN = float("nan")
NOT_BANDS = [(1500.0, 1500.0), (NAN, 2000.0), (1000.0, NAN), (2000.0, 1000.0), (-1.0, 500.0), (1000.0, 8000.5)]


def _tile():
    return _lib.load().cpc_bandreject_tile()


def _noise(n, w, seed, scale=0.05):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, w, generator=g) * scale).contiguous()


def _band(bands):
    return torch.tensor(bands, dtype=torch.float64, device=DEV).view(-1, 2)


def _entry(src, band, out, batch, window, half=157, beta=BETA, sr=SR, operand=None):
    """cpc_augment_bandreject itself: the status, nothing raised.  operand: (pointer, total, offsets pointer) instead of src's."""
    p, total, off = operand or (da._operand(src) if src is not None else (ptr(None), 0, ptr(None)))
    return _lib.load().cpc_augment_bandreject(p, total, off, ptr(band), half, beta, sr, ptr(out), batch, window,
                                              stream_ptr(torch.device(DEV)))


def _filter(src, bands, window, half=157, beta=BETA):
    """y [b, W] of the C entry on a [b, W] device buffer or FlatWindows, NaN-filled beforehand."""
    b = len(bands)
    out = torch.full((b, window), NAN, device=DEV)
    assert _entry(src, _band(bands), out, b, window, half, beta) == 0, _lib.load().cpc_last_error()
    return out


@functools.lru_cache(maxsize=None)
def _taps_gpu(half, beta=BETA, bands=tuple(BANDS)):
    """h[0 .. half] of every band from cpc_bandreject_taps, [n, half + 1] float64 on the host."""
    out = torch.full((len(bands), half + 1), NAN, dtype=torch.float64, device=DEV)
    status = _lib.load().cpc_bandreject_taps(ptr(_band(list(bands))), len(bands), half, beta, SR, ptr(out), stream_ptr(torch.device(DEV)))
    assert status == 0, _lib.load().cpc_last_error()
    return out.cpu().numpy()


# ----------------------------------------------------------------------------- the design
@pytest.mark.parametrize("half", HALVES)
def test_every_tap_is_within_2_to_the_minus_40_of_the_statement(half):
    got = _taps_gpu(half)
    assert np.isfinite(got).all()
    for row, (low, high) in enumerate(BANDS):
        want = BO.taps(low, high, half, BETA)[half:]
        err = float(np.abs(got[row] - want).max())
        print(f"half = {half}, band = ({low}, {high}): max |tap - statement| = {err:.3e} = 2^{np.log2(max(err, 1e-300)):.1f}")
        assert err <= 2.0 ** -40, (half, low, high, err)
    assert got[0, 0] == 1.0 and not got[0, 1:].any()                 # low == high: exactly the identity
    other = _taps_gpu(half, 5.65326, ((1000.0, 2000.0), (1500.0, 1500.0), (NAN, 3.0), (5.0, 4.0)))      # another beta; no bands
    assert np.abs(other[0] - BO.taps(1000.0, 2000.0, half, 5.65326)[half:]).max() <= 2.0 ** -40
    for row in (1, 2, 3):
        assert other[row, 0] == 1.0 and not other[row, 1:].any()


# ----------------------------------------------------------------------------- exact
@pytest.mark.parametrize("half", [157, 1024])
def test_an_impulse_comes_back_as_the_rounded_taps(half):
    tile = _tile()
    w = 2 * tile + 3
    bands = [(1000.0, 2000.0), (0.12, 7999.5), (0.0, 500.0)]
    taps = _taps_gpu(half, BETA, tuple(bands))
    for p in (0, half, tile - 1, tile, w - 1):
        x = torch.zeros(len(bands), w)
        x[:, p] = 1.0
        y = _filter(x.to(DEV), bands, w, half).cpu().numpy()
        dist = np.abs(np.arange(w) - p)
        for row in range(len(bands)):
            want = np.where(dist <= half, taps[row][np.minimum(dist, half)].astype(np.float32), np.float32(0))
            assert np.array_equal(y[row], want), (half, p, row, np.argwhere(y[row] != want)[:4].tolist())


def test_identity_rows_come_back_bit_for_bit_beside_filtered_rows():
    tile = _tile()
    w = tile + 77
    bands = [(1000.0, 2000.0)] + NOT_BANDS + [(0.0, 500.0)]
    x = _noise(len(bands), w, 11)
    x[2, 5] = -0.0                                                   # a copy keeps the sign of a zero; x + 0 would too, 1 x + 0 not always
    x[3, 7] = 1e-42                                                  # and a subnormal
    y = _filter(x.to(DEV), bands, w)
    want = BO.bandreject(x.numpy(), [b[0] for b in bands], [b[1] for b in bands], 157, BETA)
    for row in range(1, 1 + len(NOT_BANDS)):
        assert np.array_equal(y[row].cpu().numpy().view(np.int32), x[row].numpy().view(np.int32)), bands[row]
    for row in (0, len(bands) - 1):
        got = y[row].cpu().numpy()
        assert not np.array_equal(got, x[row].numpy()) and np.abs(got - want[row]).max() < 1e-6


def test_zero_in_zero_out():
    tile = _tile()
    for w, half in ((1, 157), (tile + 1, 157), (tile + 1, 1024), (3, 1)):
        y = _filter(torch.zeros(3, w, device=DEV), [(1000.0, 2000.0), (0.0, 8000.0), (5.0, 5.0)], w, half)
        assert not y.any() and torch.isfinite(y).all()


@pytest.mark.parametrize("half", [1, 157, 1024])
def test_window_lengths_around_the_half_length_and_the_tile(half):
    tile = _tile()
    bands = [(1000.0, 2000.0), (0.0, 8000.0), (300.0, 300.0)]
    for w in (1, half, tile - 1, tile + 1):
        x = _noise(3, w, 100 + w)
        _hold(x, bands, w, half)


def test_a_rows_bits_do_not_depend_on_batch_pack_or_launch():
    tile = _tile()
    w, pad = tile + 301, 333
    bands = [(1000.0, 2000.0), (0.0, 500.0), (4000.0, 4000.0), (7000.0, 8000.0), (3000.0, 3010.0)]
    x = _noise(5, w, 7)
    batch = _filter(x.to(DEV), bands, w)
    assert torch.equal(batch, _filter(x.to(DEV), bands, w))                              # two launches, the same bits
    for i, band in enumerate(bands):
        alone = _filter(x[i:i + 1].contiguous().to(DEV), [band], w)
        assert torch.equal(alone[0], batch[i]), f"row {i} alone"
    # the same windows inside a pack whose every other sample is NaN, in another order
    vector = torch.full((pad + 5 * (w + pad),), NAN)
    order = [3, 0, 4, 2, 1]
    offsets = torch.tensor([pad + k * (w + pad) for k in range(5)], dtype=torch.int64)
    for k, i in enumerate(order):
        vector[offsets[k]:offsets[k] + w] = x[i]
    packed = _filter(da.FlatWindows(vector.to(DEV), offsets.to(DEV)), [bands[i] for i in order], w)
    assert torch.isfinite(packed).all()
    for k, i in enumerate(order):
        assert torch.equal(packed[k], batch[i]), f"row {i} from the pack"


def test_windows_hanging_over_either_end_read_zeros():
    w, n = 700, 1000
    vector = _noise(1, n, 9)[0]
    offsets = [-w - 5, -300, 0, n - w, n - 200, n, n + 50]
    bands = [(1000.0, 2000.0), (0.0, 500.0), (7000.0, 8000.0), (1000.0, 2000.0), (6.0, 6.0), (0.0, 500.0), (1000.0, 2000.0)]
    rows = torch.zeros(len(offsets), w)
    for i, o in enumerate(offsets):
        lo, hi = max(o, 0), min(o + w, n)
        if lo < hi:
            rows[i, lo - o:hi - o] = vector[lo:hi]
    flat = da.FlatWindows(vector.to(DEV), torch.tensor(offsets, dtype=torch.int64, device=DEV))
    got = _filter(flat, bands, w)
    assert torch.equal(got, _filter(rows.to(DEV), bands, w))
    assert not got[0].any() and not got[5].any() and not got[6].any() and got[1].any() and got[4].any()


def test_out_is_fully_overwritten_and_its_guard_band_is_untouched():
    tile = _tile()
    b, guard = 4, 2048
    bands = [(1000.0, 2000.0), (0.0, 500.0), (9.0, 9.0), (7000.0, 8000.0)]
    for w in (tile + 5, 257, 1):
        x = _noise(b, w, 41).to(DEV)
        ybuf = torch.full((guard + b * w + guard,), NAN, device=DEV)
        out = ybuf[guard:guard + b * w].view(b, w)
        assert _entry(x, _band(bands), out, b, w) == 0
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        assert torch.isnan(ybuf[:guard]).all() and torch.isnan(ybuf[guard + b * w:]).all()
        assert torch.equal(out, _filter(x, bands, w))


def test_every_refusal_leaves_out_untouched():
    lib = _lib.load()
    b, w = 3, 512
    x = _noise(b, w, 51).to(DEV)
    band = _band([(1000.0, 2000.0)] * b)
    out = torch.full((b, w), NAN, device=DEV)
    taps = torch.full((b, 158), NAN, dtype=torch.float64, device=DEV)
    inf = float("inf")

    def refused(status, word="augment_bandreject:"):
        torch.cuda.synchronize()
        assert status == -1 and lib.cpc_last_error().startswith(word.encode()), (status, lib.cpc_last_error())
        assert torch.isnan(out).all() and torch.isnan(taps).all()

    def design(batch=b, half=157, beta=BETA, sr=SR, band=band, taps=taps):
        return lib.cpc_bandreject_taps(ptr(band), batch, half, beta, sr, ptr(taps), stream_ptr(torch.device(DEV)))

    for bad in (0, -5):
        refused(_entry(x, band, out, b, bad))
    for bad in (-1, 65536):
        refused(_entry(x, band, out, bad, w))
        refused(design(batch=bad), "bandreject_taps:")
    for bad in (0, -1, 1025):
        refused(_entry(x, band, out, b, w, half=bad))
        refused(design(half=bad), "bandreject_taps:")
    for bad in (NAN, inf, -0.1, 50.1):
        refused(_entry(x, band, out, b, w, beta=bad))
        refused(design(beta=bad), "bandreject_taps:")
    for bad in (NAN, inf, 0.0, -16000.0):
        refused(_entry(x, band, out, b, w, sr=bad))
        refused(design(sr=bad), "bandreject_taps:")
    refused(_entry(None, band, out, b, w))
    refused(_entry(x, None, out, b, w))
    refused(design(band=None), "bandreject_taps:")
    refused(design(taps=None), "bandreject_taps:")
    offsets = torch.zeros(b, dtype=torch.int64, device=DEV)                                # offsets without the vector's length
    refused(_entry(x, band, out, b, w, operand=(ptr(x), 0, ptr(offsets))))
    same = x.clone()
    assert _entry(same, band, same, b, w) == -1 and b"must not be the input" in lib.cpc_last_error()
    assert _entry(x, band, None, b, w) == -1 and b"null pointer" in lib.cpc_last_error()
    torch.cuda.synchronize()
    assert torch.equal(same, x) and torch.isnan(out).all()
    # b == 0: nothing to do, nothing done -- with or without pointers
    assert _entry(x, band, out, 0, w) == 0 and _entry(None, None, None, 0, w) == 0 and design(batch=0) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(taps).all()
    with pytest.raises(ValueError, match="^high "):
        audio.bandreject(x, 100.0, 8001.0)


# ----------------------------------------------------------------------------- accuracy
def _within(got, y64, x, half):
    """The bound, every sample: |y - y64| <= 2^-24 |y64| + 2^-38 sum_j |x[t - j]| + 2^-149.  Returns the worst error / bound."""
    assert got.shape == y64.shape and got.dtype == np.float32 and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - y64)
    bound = 2.0 ** -24 * np.abs(y64) + 2.0 ** -38 * BO.reach(x, half) + 2.0 ** -149
    ratio = float((err / bound).max())
    print(f"shape {got.shape}, half = {half}: max |kernel - f64| = {err.max():.3e}, worst error / bound = {ratio:.3f}")
    assert (err <= bound).all(), (got.shape, half, ratio, np.argwhere(err > bound)[:4].tolist())
    return ratio


def _hold(x, bands, w, half, beta=BETA):
    y64 = BO.bandreject(x.numpy(), [b[0] for b in bands], [b[1] for b in bands], half, beta)
    got = _filter(x.to(DEV), bands, w, half, beta).cpu().numpy()
    _within(got, y64, x.numpy(), half)
    return got, y64


@pytest.mark.parametrize("half,tiles,extra", [(157, 3, 5), (1024, 2, 3), (1, 2, 3)])
def test_every_sample_holds_the_bound_and_the_stop_band_is_118_dB_down(half, tiles, extra):
    w = tiles * _tile() + extra
    bands = [(0.0, 500.0), (7000.0, 8000.0), (3000.0, 3010.0), (0.0, 8000.0), (0.12, 7999.5), (2552.328389222971, 2722.165046087116),
             (1000.0, 2000.0), (1000.0, 2000.0)]
    x = _noise(len(bands), w, 1000 + half)
    x[-1] = torch.from_numpy((0.5 * np.sin(2 * np.pi * 1500.0 * np.arange(w) / SR)).astype(np.float32))      # 1500 Hz under (1000, 2000)
    got, _y64 = _hold(x.contiguous(), bands, w, half)
    if half > 1:              # (three taps have no stop band: with half = 1 the transition is as wide as the whole spectrum)
        inside = np.abs(got[-1, half:w - half]).max()
        print(f"the sine's remainder inside [half, W - half): {inside:.3e} against {0.5 * 10 ** (-118 / 20):.3e}")
        assert inside <= 0.5 * 10 ** (-118 / 20)


# ----------------------------------------------------------------------------- the transform and the direct call
def test_the_transform_the_direct_call_and_the_replay_agree_bit_for_bit():
    w = 2048
    case, = [c for c in GOLDEN["cases"] if c["seed"] == 1234 and c["scaler"] == 1.0]
    np.random.seed(1234)
    aug = da.BandrejectSincAugment()
    x = _noise(6, w, 62).to(DEV)
    kept = x.clone()
    y = aug(x.view(6, 1, w))
    assert y.shape == (6, 1, w) and torch.equal(x, kept)
    plan = aug.last_plan
    assert plan["band"].tolist() == case["pairs"][:6] and plan["low"].tolist() == [p[0] for p in case["pairs"][:6]]
    np.random.seed(1234)
    bands = [BO.draw() for _ in range(6)]
    assert torch.equal(y.view(6, w), _filter(kept, bands, w))                           # the C entry on the oracle's draws
    _within(y.view(6, w).cpu().numpy(), BO.apply_plan(plan, 0, 6, kept.cpu().numpy()), kept.cpu().numpy(), 157)
    assert torch.equal(aug.apply(plan, 0, 6, kept.clone()), y.view(6, w))               # the same plan again: the same bits
    part = aug.apply(plan, 2, 5, kept[2:5].contiguous())                                # rows of a plan
    assert torch.equal(part, y.view(6, w)[2:5])
    dst = torch.full((6, w), NAN, device=DEV)
    assert aug.apply(plan, 0, 6, kept, dst) is dst and torch.equal(dst, y.view(6, w))
    flat = da.FlatWindows(kept.view(-1), torch.arange(6, device=DEV, dtype=torch.int64) * w)
    assert torch.equal(aug.apply(plan, 0, 6, flat, window=w), y.view(6, w))
    one = aug(kept[0].view(1, w))                                                      # the reference's single [1, W] window
    low, high = aug.last_plan["band"][0]
    assert one.shape == (1, w) and torch.equal(one, audio.bandreject(kept[0].view(1, w), low, high))
    # the direct call: one pair for all rows, one per row, [b, 1, W] / [b, W] / [W]
    assert torch.equal(audio.bandreject(kept, plan["low"], plan["high"]), y.view(6, w))
    assert torch.equal(audio.bandreject(kept.view(6, 1, w), torch.from_numpy(plan["low"]), list(plan["high"])), y)
    same_band = audio.bandreject(kept.view(2, 3, w), 1000.0, 2000.0)
    assert same_band.shape == (2, 3, w) and torch.equal(same_band.view(6, w), _filter(kept, [(1000.0, 2000.0)] * 6, w))
    assert torch.equal(audio.bandreject(kept[4], 1000.0, 2000.0), same_band.view(6, w)[4])
    assert torch.equal(audio.bandreject(kept, 1000.0, plan["high"].clip(1000.0)), _filter(kept, [(1000.0, max(h, 1000.0)) for h in plan["high"]], w))
    short = audio.bandreject(kept, 1000.0, 2000.0, attenuation_dB=60.0)
    assert torch.equal(short, _filter(kept, [(1000.0, 2000.0)] * 6, w, 73, BO.design(60.0)[0])) and not torch.equal(short, same_band.view(6, w))
    assert torch.equal(audio.bandreject(kept, 700.0, 700.0), kept)
    with pytest.raises(ValueError, match="5 low edges for 6 rows"):
        audio.bandreject(kept, [1.0, 2.0, 3.0, 4.0, 5.0], 8000.0)
    with pytest.raises(ValueError, match="7 high edges for 6 rows"):
        audio.bandreject(kept, 0.0, [8000.0] * 7)


def test_bandreject_then_time_dropout_lands_in_dst():
    w = 2048
    np.random.seed(63)
    kept = _noise(6, w, 64).to(DEV)
    both = da.CombinedTransforms(["bandreject_sinc", "time_dropout"], t_ms=20, bandreject_scaler=2.0)
    z = both(kept.view(6, 1, w)).view(6, w)
    reject, drop = both.last_plan["parts"]
    assert reject["kind"] == "bandreject_sinc" and drop["kind"] == "time_dropout"
    alone = da.BandrejectSincAugment(2.0).apply(reject, 0, 6, kept.clone())
    assert not torch.equal(alone, kept)
    by_hand = alone.clone()
    for i in range(6):
        s, n = int(drop["start"][i]), int(drop["length"][i])
        by_hand[i, s:s + n] = 0
    assert torch.equal(z, by_hand) and drop["length"].max() > 0
    dst = torch.full((6, w), NAN, device=DEV)
    got = both.apply(both.last_plan, 0, 6, kept, dst)
    assert got is dst and torch.equal(dst, by_hand)
    flat = da.FlatWindows(kept.view(-1), torch.arange(6, device=DEV, dtype=torch.int64) * w)
    dst.fill_(NAN)
    assert both.apply(both.last_plan, 0, 6, flat, dst) is dst and torch.equal(dst, by_hand)


# ----------------------------------------------------------------------------- the feeder and the command line
def _seed(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def test_feeder_yields_the_replay_of_the_plan_it_drew():
    w = 2 * _tile()
    _seed(71)
    aug = da.BandrejectSincAugment()
    seqs, speakers = ds.findAllSeqs(DB, extension=".flac")
    seqs = sorted(seqs, key=lambda s: s[1])
    speech = ds.AudioBatchData(DB, w, seqs, None, len(speakers), device=DEV, augmentation=aug, augment_past=True)
    loader = speech.getDataLoader(8, "samespeaker", True)
    out = [(s.clone(), l.clone()) for s, l in loader]
    pack, = loader.plans
    assert pack["future"] is None and pack["past"]["kind"] == "bandreject_sinc" and len(out) == len(pack["batches"]) > 2
    flat = speech.data.cpu()
    row = 0
    for i, ((seq, _label), offsets) in enumerate(zip(out, pack["batches"])):
        b = len(offsets)
        clean = torch.stack([flat[o:o + w] for o in offsets])
        assert seq.shape == (b, 2, 1, w) and torch.equal(seq[:, 1, 0].cpu(), clean)      # the future half stays clean
        replay = aug.apply(pack["past"], row, row + b, clean.to(DEV))
        assert torch.equal(seq[:, 0, 0], replay), f"batch {i}"
        if i == 0:
            _within(seq[:, 0, 0].cpu().numpy(), BO.apply_plan(pack["past"], row, row + b, clean.numpy()), clean.numpy(), 157)
            assert not torch.equal(seq[:, 0, 0].cpu(), clean)
        row += b
    past = pack["past"]
    assert row == past["n"] and 0 <= past["low"].min() and past["high"].max() <= 8000 and (past["low"] < past["high"]).all()


def test_main_trains_with_bandreject_sinc(tmp_path, monkeypatch):
    seen = []
    original = ds.AudioBatchData.augmented_from

    def watched(self, *a, **k):
        seen.append(type(self.augmentation).__name__)
        return original(self, *a, **k)

    monkeypatch.setattr(ds.AudioBatchData, "augmented_from", watched)
    run_dir = str(tmp_path / "bandreject")
    os.makedirs(run_dir)
    argv = ["--pathDB", DB, "--pathCheckpoint", os.path.join(run_dir, "run"), "--path_cache", os.path.join(run_dir, "seqs_cache.txt"),
            "--hiddenEncoder", "64", "--hiddenGar", "64", "--nPredicts", "4", "--negativeSamplingExt", "16", "--arMode", "GRU",
            "--rnnMode", "linear", "--batchSizeGPU", "8", "--nGPU", "1", "--random_seed", "0", "--save_step", "1",
            "--pathTrain", SEQ_LIST, "--pathVal", SEQ_LIST, "--nEpoch", "1", "--sizeWindow", "5120",
            "--augment_past", "--augment_type", "bandreject_sinc"]
    res = tr.main(argv)
    assert res.logs["epoch"] == [0] and len(seen) >= 2 and seen[0] == "BandrejectSincAugment"
    for key in ("locLoss_train", "locLoss_val"):
        assert len(res.logs[key]) == 1 and np.isfinite(np.asarray(res.logs[key], dtype=np.float64)).all(), key
    with open(os.path.join(run_dir, "run", "checkpoint_args.json")) as fh:
        written = json.load(fh)
    assert written["augment_type"] == ["bandreject_sinc"] and written["augment_past"] is True
