"""The `freeverb` kernel (csrc/freeverb.hip) against the numpy statement of tests/freeverb_oracle.py.  Exact properties by
equality (where every delay sits, zero in / zero out, what the definition promises about packs, batches, launches and guard
bands, the refusals of the C entry); accuracy against the float64 evaluation with the float32 evaluation's own error E32 as the
yardstick, max |y_gpu - y64| <= 4 max(E32, 2^-24 max |y64|) per case; then the transform, the direct call, the feeder and the
command line.

The kernel keeps the statement's operations and their order (the file is built without contraction), so beyond the bound above its
output is expected to EQUAL the float32 evaluation; the accuracy test asserts that too."""
import ctypes
import functools
import json
import os
import random

import numpy as np
import pytest
import torch

import freeverb_oracle as FO
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
DEV = "cuda:0"
ROOMS = [0, 1, 50, 98, 99]
G32 = np.float32(0.015)


def _noise(n, w, seed, scale=0.05):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, w, generator=g) * scale).contiguous()


def _entry(src, comb_len, out, batch, window, bound=None, allpass=None, fb=None, dmp=None, g=None, operand=None,
           params=(100.0, 100.0, 0.0)):
    """cpc_augment_freeverb itself: the status, nothing raised.  operand: (pointer, total, offsets pointer) instead of src's."""
    p, total, off = operand or (da._operand(src) if src is not None else (ptr(None), 0, ptr(None)))
    f, d, gg = (float(np.float32(v)) for v in FO.scalars(*params))
    allpass = FO.allpass_lengths() if allpass is None else allpass
    ap = (ctypes.c_int * 4)(*allpass) if allpass != "null" else None
    bound = int(comb_len.max()) if bound is None else bound
    return _lib.load().cpc_augment_freeverb(p, total, off, ptr(comb_len), bound, ap, f if fb is None else fb, d if dmp is None else dmp,
                                            gg if g is None else g, ptr(out), batch, window, stream_ptr(torch.device(DEV)))


def _table(rooms):
    return torch.tensor([FO.comb_lengths(int(r)) for r in rooms], dtype=torch.int32, device=DEV).view(-1, 8)


def _reverb(src, rooms, window, params=(100.0, 100.0, 0.0)):
    """y [b, W] of the C entry on a [b, W] device buffer or FlatWindows, NaN-filled beforehand."""
    b = len(rooms)
    out = torch.full((b, window), float("nan"), device=DEV)
    assert _entry(src, _table(rooms), out, b, window, params=params) == 0, _lib.load().cpc_last_error()
    return out


# ----------------------------------------------------------------------------- exact
def test_a_unit_impulse_pins_every_delay():
    w = 1300
    x = torch.zeros(len(ROOMS), w)
    x[:, 0] = 1.0
    y = _reverb(x.to(DEV), ROOMS, w).cpu().numpy()
    want = FO.freeverb(x.numpy(), ROOMS, dtype=np.float32)
    for row, rs in enumerate(ROOMS):
        lengths = FO.comb_lengths(rs)
        assert y[row, 0] == 1.0 and not y[row, 1:lengths[0]].any(), rs
        assert y[row, lengths[0]] == G32, (rs, lengths[0], y[row, lengths[0]])
        # every comb's first echo arrives where its length says (the float32 statement puts something there, and so does the kernel),
        # and every all-pass's: the first comb echo comes again A[a] samples later
        for n in lengths + tuple(lengths[0] + a for a in FO.allpass_lengths()):
            if n < w:
                assert want[row, n] != 0 and y[row, n] == want[row, n], (rs, n)
    assert np.array_equal(y, want)                                   # all of it, bit for bit (no sample of an impulse response is spared)


def test_zero_in_zero_out_and_short_windows_come_back():
    for w in (1, 40, 1300):
        y = _reverb(torch.zeros(3, w, device=DEV), [0, 50, 99], w)
        assert not y.any() and torch.isfinite(y).all()
    for rs in ROOMS:
        first = FO.comb_lengths(rs)[0]
        for w in (1, first - 1, first):
            x = _noise(2, w, 100 * rs + w).to(DEV)
            assert torch.equal(_reverb(x, [rs, rs], w), x), (rs, w)


def test_a_rows_bits_do_not_depend_on_batch_pack_or_launch():
    w, pad = 1300, 333
    rooms = [99, 0, 50, 1, 98]
    x = _noise(5, w, 7)
    batch = _reverb(x.to(DEV), rooms, w)
    assert torch.equal(batch, _reverb(x.to(DEV), rooms, w))                               # two launches, the same bits
    for i, rs in enumerate(rooms):
        alone = _reverb(x[i:i + 1].contiguous().to(DEV), [rs], w)
        assert torch.equal(alone[0], batch[i]), f"row {i} alone"
    # the same windows inside a pack whose every other sample is NaN, in another order
    vector = torch.full((pad + 5 * (w + pad),), float("nan"))
    order = [3, 0, 4, 2, 1]
    offsets = torch.tensor([pad + k * (w + pad) for k in range(5)], dtype=torch.int64)
    for k, i in enumerate(order):
        vector[offsets[k]:offsets[k] + w] = x[i]
    packed = _reverb(da.FlatWindows(vector.to(DEV), offsets.to(DEV)), [rooms[i] for i in order], w)
    assert torch.isfinite(packed).all()
    for k, i in enumerate(order):
        assert torch.equal(packed[k], batch[i]), f"row {i} from the pack"


def test_windows_hanging_over_either_end_read_zeros():
    w, n = 700, 1000
    vector = _noise(1, n, 9)[0]
    offsets = [-w - 5, -300, 0, n - w, n - 200, n, n + 50]
    rooms = [0, 99, 50, 1, 98, 0, 99]
    rows = torch.zeros(len(offsets), w)
    for i, o in enumerate(offsets):
        lo, hi = max(o, 0), min(o + w, n)
        if lo < hi:
            rows[i, lo - o:hi - o] = vector[lo:hi]
    flat = da.FlatWindows(vector.to(DEV), torch.tensor(offsets, dtype=torch.int64, device=DEV))
    got = _reverb(flat, rooms, w)
    assert torch.equal(got, _reverb(rows.to(DEV), rooms, w))
    assert not got[0].any() and not got[5].any() and not got[6].any() and got[1].any()


def test_out_is_fully_overwritten_and_its_guard_band_is_untouched():
    b, guard = 5, 1024
    for w in (1300, 257, 1):
        x = _noise(b, w, 41).to(DEV)
        ybuf = torch.full((guard + b * w + guard,), float("nan"), device=DEV)
        out = ybuf[guard:guard + b * w].view(b, w)
        assert _entry(x, _table(ROOMS), out, b, w) == 0
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        assert torch.isnan(ybuf[:guard]).all() and torch.isnan(ybuf[guard + b * w:]).all()
        assert torch.equal(out, _reverb(x, ROOMS, w))


def test_a_bad_table_is_clamped_into_the_lines():
    # lengths outside [1, len_bound] are clamped on the device: the result is that of the clamped table
    w = 600
    x = _noise(3, w, 43).to(DEV)
    bad = torch.tensor([[0, -7, 5000, 59, 1 << 30, -(1 << 30), 3, 1], [40, 43, 46, 49, 52, 54, 56, 59], [1] * 8], dtype=torch.int32,
                       device=DEV)
    clamped = bad.clamp(1, 59)
    out = torch.full((3, w), float("nan"), device=DEV)
    assert _entry(x, bad, out, 3, w, bound=59) == 0
    want = FO.freeverb(x.cpu().numpy(), None, dtype=np.float32, comb_len=clamped.cpu().numpy())
    assert np.array_equal(out.cpu().numpy(), want)
    # the longest lines the entry takes: len_bound = 1024 and all-passes of 1024
    long = torch.full((1, 8), 1024, dtype=torch.int32, device=DEV)
    out = torch.full((1, w), float("nan"), device=DEV)
    assert _entry(x[:1], long, out, 1, w, bound=1024, allpass=(1024, 1024, 1024, 1024)) == 0
    assert torch.equal(out, x[:1])                                   # (nothing comes back within 600 samples)


def test_every_refusal_leaves_out_untouched():
    lib = _lib.load()
    b, w = 3, 512
    x = _noise(b, w, 51).to(DEV)
    table = _table([0, 50, 99])
    out = torch.full((b, w), float("nan"), device=DEV)
    nan, inf = float("nan"), float("inf")

    def refused(status, word="augment_freeverb"):
        torch.cuda.synchronize()
        assert status == -1 and word.encode() in lib.cpc_last_error(), (status, lib.cpc_last_error())
        assert torch.isnan(out).all()

    refused(_entry(x, table, out, b, 0))
    refused(_entry(x, table, out, b, -5))
    refused(_entry(x, table, out, -1, w))
    refused(_entry(x, table, out, 65536, w))
    refused(_entry(x, table, out, b, w, bound=0), "len_bound")
    refused(_entry(x, table, out, b, w, bound=1025), "len_bound")
    refused(_entry(x, table, out, b, w, allpass=(82, 124, 0, 202)), "allpass_len[2]")
    refused(_entry(x, table, out, b, w, allpass=(1025, 124, 160, 202)), "allpass_len[0]")
    refused(_entry(x, table, out, b, w, allpass="null"), "all-pass")
    for bad in (1.0, 1.5, -0.1):
        refused(_entry(x, table, out, b, w, fb=bad), "feedback")
    for bad in (1.1, -0.1):
        refused(_entry(x, table, out, b, w, dmp=bad), "damping")
    for bad in (nan, inf, -inf):
        refused(_entry(x, table, out, b, w, fb=bad), "not finite")
        refused(_entry(x, table, out, b, w, dmp=bad), "not finite")
        refused(_entry(x, table, out, b, w, g=bad), "not finite")
    refused(_entry(None, table, out, b, w), "null pointer")
    refused(_entry(x, None, out, b, w, bound=581), "null pointer")
    offsets = torch.zeros(b, dtype=torch.int64, device=DEV)                                # offsets without the vector's length
    refused(_entry(x, table, out, b, w, operand=(ptr(x), 0, ptr(offsets))), "vector's length")
    same = x.clone()
    assert _entry(same, table, same, b, w) == -1 and b"must not be the input" in lib.cpc_last_error()
    assert _entry(x, table, None, b, w) == -1 and b"null pointer" in lib.cpc_last_error()
    torch.cuda.synchronize()
    assert torch.equal(same, x) and torch.isnan(out).all()
    # b == 0: nothing to do, nothing done -- with or without pointers
    assert _entry(x, table, out, 0, w) == 0 and _entry(None, None, None, 0, w, bound=581) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    with pytest.raises(ValueError, match="room size"):
        audio.freeverb(x, 101)


# ----------------------------------------------------------------------------- accuracy
def _inputs(w, seed):
    """Rows of 0.05 randn, one low-frequency sine and one constant 0.5, with mixed rooms."""
    rooms = ROOMS + [37, 73, 99]
    x = _noise(len(rooms), w, seed)
    x[-2] = 0.2 * torch.sin(2 * np.pi * 60.0 * torch.arange(w, dtype=torch.float32) / 16000.0)
    x[-1] = 0.5
    return x.contiguous(), rooms


@functools.lru_cache(maxsize=None)
def _case(w, params, big=False):
    """(x, rooms, y64, y32) of one accuracy case: the statement runs once per case, whoever asks."""
    if big:
        x, rooms = _noise(3, w, 5), [99, 0, 50]
    else:
        x, rooms = _inputs(w, 1000 + w)
    y64 = FO.freeverb(x.numpy(), rooms, *params, dtype=np.float64)
    y32 = FO.freeverb(x.numpy(), rooms, *params, dtype=np.float32)
    return x, rooms, y64, y32


def _hold(w, params, big=False):
    x, rooms, y64, y32 = _case(w, params, big)
    got = _reverb(x.to(DEV), rooms, w, params).cpu().numpy()
    assert np.isfinite(got).all()
    e32 = float(np.abs(y32.astype(np.float64) - y64).max())
    yard = max(e32, 2.0 ** -24 * float(np.abs(y64).max()))
    err = float(np.abs(got.astype(np.float64) - y64).max())
    same = np.array_equal(got, y32)
    print(f"W = {w}, b = {len(rooms)}, (reverberance, hf_damping, dB) = {params}: max |kernel - f64| = {err:.3e}, E32 = {e32:.3e}, "
          f"2^-24 max|y| = {2.0 ** -24 * float(np.abs(y64).max()):.3e}, ratio = {err / yard:.3f}, equals the f32 statement: {same}")
    assert err <= 4 * yard, f"W = {w}: error / yardstick = {err / yard:.3f}"
    assert same, (f"W = {w}: {int((got != y32).sum())} samples differ from the float32 statement, first at "
                  f"{np.argwhere(got != y32)[:4].tolist()}")
    return err / yard


@pytest.mark.parametrize("w", [1, 39, 41, 64, 583, 1300, 4096])
def test_outputs_stay_within_four_times_the_float32_statements_own_error(w):
    _hold(w, (100.0, 100.0, 0.0))


def test_reverb_dropouts_parameters_hold_too():
    _hold(1300, (50.0, 50.0, 0.0))
    _hold(583, (30.0, 0.0, -6.0))


def test_full_length_windows_hold():
    _hold(20480, (100.0, 100.0, 0.0), big=True)


# ----------------------------------------------------------------------------- the transform and the direct call
def test_the_transform_the_direct_call_and_the_replay_agree_bit_for_bit():
    w = 2048
    np.random.seed(61)
    aug = da.FreeverbAugment()
    x = _noise(6, w, 62).to(DEV)
    kept = x.clone()
    y = aug(x.view(6, 1, w))
    assert y.shape == (6, 1, w) and torch.equal(x, kept)
    plan = aug.last_plan
    np.random.seed(61)
    assert plan["room"].tolist() == [int(np.random.randint(0, 100)) for _ in range(6)]
    assert np.array_equal(y.view(6, w).cpu().numpy(), FO.apply_plan(plan, 0, 6, kept.cpu().numpy(), dtype=np.float32))
    assert torch.equal(aug.apply(plan, 0, 6, kept.clone()), y.view(6, w))               # the same plan again: the same bits
    part = aug.apply(plan, 2, 5, kept[2:5].contiguous())                                # rows of a plan
    assert torch.equal(part, y.view(6, w)[2:5])
    dst = torch.full((6, w), float("nan"), device=DEV)
    assert aug.apply(plan, 0, 6, kept, dst) is dst and torch.equal(dst, y.view(6, w))
    flat = da.FlatWindows(kept.view(-1), torch.arange(6, device=DEV, dtype=torch.int64) * w)
    assert torch.equal(aug.apply(plan, 0, 6, flat, window=w), y.view(6, w))
    one = aug(kept[0].view(1, w))                                                      # the reference's single [1, W] window
    assert one.shape == (1, w) and torch.equal(one, audio.freeverb(kept[0].view(1, w), int(aug.last_plan["room"][0])))
    # the direct call: one int for all rows, one value per row, [b, 1, W] / [b, W] / [W]
    rows = audio.freeverb(kept, plan["room"])
    assert torch.equal(rows, y.view(6, w))
    assert torch.equal(audio.freeverb(kept.view(6, 1, w), torch.from_numpy(plan["room"])), y)
    same_room = audio.freeverb(kept.view(2, 3, w), 57)
    assert same_room.shape == (2, 3, w) and torch.equal(same_room.view(6, w), _reverb(kept, [57] * 6, w))
    assert torch.equal(audio.freeverb(kept[4], 57), same_room.view(6, w)[4])
    half = audio.freeverb(kept, 57, reverberance=50, hf_damping=50)
    assert torch.equal(half, _reverb(kept, [57] * 6, w, (50.0, 50.0, 0.0))) and not torch.equal(half, same_room.view(6, w))
    with pytest.raises(ValueError, match="5 room sizes for 6 rows"):
        audio.freeverb(kept, [1, 2, 3, 4, 5])
    with pytest.raises(TypeError, match="whole numbers"):
        audio.freeverb(kept, 1.5)


def test_freeverb_then_time_dropout_lands_in_dst():
    w = 2048
    np.random.seed(63)
    kept = _noise(6, w, 64).to(DEV)
    both = da.CombinedTransforms(["freeverb", "time_dropout"], t_ms=20)
    z = both(kept.view(6, 1, w)).view(6, w)
    reverb, drop = both.last_plan["parts"]
    assert reverb["kind"] == "freeverb" and drop["kind"] == "time_dropout"
    alone = da.FreeverbAugment().apply(reverb, 0, 6, kept.clone())
    by_hand = alone.clone()
    for i in range(6):
        s, n = int(drop["start"][i]), int(drop["length"][i])
        by_hand[i, s:s + n] = 0
    assert torch.equal(z, by_hand) and drop["length"].max() > 0
    dst = torch.full((6, w), float("nan"), device=DEV)
    got = both.apply(both.last_plan, 0, 6, kept, dst)
    assert got is dst and torch.equal(dst, by_hand)
    flat = da.FlatWindows(kept.view(-1), torch.arange(6, device=DEV, dtype=torch.int64) * w)
    dst.fill_(float("nan"))
    assert both.apply(both.last_plan, 0, 6, flat, dst) is dst and torch.equal(dst, by_hand)


# ----------------------------------------------------------------------------- the feeder and the command line
def _seed(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def test_feeder_yields_the_replay_of_the_plan_it_drew(capsys):
    w = 20480
    _seed(71)
    aug = da.FreeverbAugment()
    seqs, speakers = ds.findAllSeqs(DB, extension=".flac")
    seqs = sorted(seqs, key=lambda s: s[1])
    speech = ds.AudioBatchData(DB, w, seqs, None, len(speakers), device=DEV, augmentation=aug, augment_past=True)
    loader = speech.getDataLoader(8, "samespeaker", True)
    out = [(s.clone(), l.clone()) for s, l in loader]
    pack, = loader.plans
    assert pack["future"] is None and pack["past"]["kind"] == "freeverb" and len(out) == len(pack["batches"]) > 2
    flat = speech.data.cpu()
    row = 0
    for i, ((seq, _label), offsets) in enumerate(zip(out, pack["batches"])):
        b = len(offsets)
        clean = torch.stack([flat[o:o + w] for o in offsets])
        assert seq.shape == (b, 2, 1, w) and torch.equal(seq[:, 1, 0].cpu(), clean)      # the future half stays clean
        replay = aug.apply(pack["past"], row, row + b, clean.to(DEV))
        assert torch.equal(seq[:, 0, 0], replay), f"batch {i}"
        if i == 0:                                                                      # (the statement costs a second per batch)
            want = FO.apply_plan(pack["past"], row, row + b, clean.numpy(), dtype=np.float32)
            assert np.array_equal(seq[:, 0, 0].cpu().numpy(), want)
            assert not torch.equal(seq[:, 0, 0].cpu(), clean)
        row += b
    assert row == pack["past"]["n"] and 0 <= pack["past"]["room"].min() and pack["past"]["room"].max() < 100
    assert len(set(pack["past"]["room"].tolist())) > 3


def test_main_trains_with_freeverb_and_time_dropout(tmp_path, monkeypatch, capsys):
    seen = []
    original = ds.AudioBatchData.augmented_from

    def watched(self, *a, **k):
        seen.append([type(t).__name__ for t in self.augmentation.transfors_cfgs])
        return original(self, *a, **k)

    monkeypatch.setattr(ds.AudioBatchData, "augmented_from", watched)
    run_dir = str(tmp_path / "freeverb")
    os.makedirs(run_dir)
    argv = ["--pathDB", DB, "--pathCheckpoint", os.path.join(run_dir, "run"), "--path_cache", os.path.join(run_dir, "seqs_cache.txt"),
            "--hiddenEncoder", "64", "--hiddenGar", "64", "--nPredicts", "4", "--negativeSamplingExt", "16", "--arMode", "GRU",
            "--rnnMode", "linear", "--batchSizeGPU", "8", "--nGPU", "1", "--random_seed", "0", "--save_step", "1",
            "--pathTrain", SEQ_LIST, "--pathVal", SEQ_LIST, "--nEpoch", "1",
            "--augment_past", "--augment_type", "freeverb", "time_dropout"]
    res = tr.main(argv)
    assert res.logs["epoch"] == [0] and len(seen) >= 2 and seen[0] == ["FreeverbAugment", "TimeDropoutAugment"]
    for key in ("locLoss_train", "locLoss_val"):
        assert len(res.logs[key]) == 1 and np.isfinite(np.asarray(res.logs[key], dtype=np.float64)).all(), key
    with open(os.path.join(run_dir, "run", "checkpoint_args.json")) as fh:
        written = json.load(fh)
    assert written["augment_type"] == ["freeverb", "time_dropout"] and written["augment_past"] is True
