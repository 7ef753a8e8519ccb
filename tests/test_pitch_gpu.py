"""The `pitch_wsola` kernels (csrc/pitch.hip) against the float64 statement of tests/pitch_oracle.py: the segment starts q EQUAL
the statement's -- near-ties, exact ties and all -- and every output stays within the statement's first-order bound (its
docstring derives it; the allowance for the device's f64 sin / cos in it is ASSUMED).  Then what the definition promises about
packs, batches and launches, the refusals of the C entry, the transform, the direct call, the feeder and the command line.

Worst |kernel - fp64| / bound measured on an MI355X over every case of this file: 0.32 (mixed cents, W = 2433)."""
import json
import os
import random

import numpy as np
import pytest
import torch

import pitch_oracle as PO
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
W = 2048
MIXED = [-1200, -300, -1, 0, 1, 57, 300, 1200]
Q_FILL = 0x7f7f7f7f


def _speechlike(n, w, seed, scale=0.1):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(w, dtype=torch.float32)
    return (torch.randn(n, w, generator=g) * scale * (0.3 + torch.sin(t / 700.0) ** 2)).contiguous()


def _tables(cents, window, count=None):
    host = PO.tables(cents, window, count)
    return host, {k: torch.from_numpy(v).to(DEV) for k, v in host.items()}


def _entry(src, tables, out, q, batch, window, segments=None, bound=None, operand=None):
    """cpc_augment_pitch itself: the status, nothing raised.  operand: (pointer, total, offsets pointer) instead of src's."""
    p, total, off = operand or (da._operand(src) if src is not None else (ptr(None), 0, ptr(None)))
    segments = tables["nominal"].shape[1] if segments is None else segments
    bound = int(tables["cents"].abs().max()) if bound is None else bound
    return _lib.load().cpc_augment_pitch(p, total, off, ptr(tables["ratio"]), ptr(tables["cutoff"]), ptr(tables["cents"]), bound,
                                         ptr(tables["nominal"]), segments, ptr(out), ptr(q), batch, window,
                                         stream_ptr(torch.device(DEV)))


def _shift(src, cents, window, count=None):
    """(y [b, W], q [b, J]) of the C entry on a [b, W] device buffer or FlatWindows."""
    _host, tables = _tables(cents, window, count)
    b = len(cents)
    out = torch.full((b, window), float("nan"), device=DEV)
    q = torch.full((b, tables["nominal"].shape[1]), Q_FILL, dtype=torch.int32, device=DEV)
    assert _entry(src, tables, out, q, b, window) == 0, _lib.load().cpc_last_error()
    return out, q


def _hold(y, q, x, cents, what, count=None):
    """q equal to the statement's, y within its bound; returns the worst error-to-bound ratio."""
    want, want_q, bound = PO.pitch_batch(np.asarray(x), cents, count if count is not None else q.shape[1])
    got, got_q = y.detach().double().cpu().numpy(), q.cpu().numpy().astype(np.int64)
    assert got_q.shape == want_q.shape and np.array_equal(got_q, want_q), \
        f"{what}: segment starts differ at (row, segment) {np.argwhere(got_q != want_q)[:8].tolist()}"
    assert np.isfinite(got).all(), what
    err = np.abs(got - want)
    exact = bound == 0.0
    assert not err[exact].any(), f"{what}: an output with no rounding in it (zero bound) differs"
    ratio = float((err[~exact] / bound[~exact]).max()) if (~exact).any() else 0.0
    print(f"{what}: max |kernel - fp64| = {err.max():.2e}, worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: error / bound = {ratio:.3f}"
    for i, c in enumerate(cents):
        if c == 0:
            assert np.array_equal(got[i], np.asarray(x[i], dtype=np.float64)), f"{what}: row {i} (0 cents) is not the window's bits"
    return ratio


# ----------------------------------------------------------------------------- against the statement
@pytest.mark.parametrize("w", [1, 1311, 1312, 1313, 2432, 2433, 2048])
def test_mixed_cents_in_one_batch_at_every_window_length(w):
    x = _speechlike(8, w, 100 + w)
    y, q = _shift(x.to(DEV), MIXED, w)
    _hold(y, q, x.numpy(), MIXED, f"W = {w}")


def test_training_window_of_20480_samples():
    x = _speechlike(2, 20480, 7)
    y, q = _shift(x.to(DEV), [300, -300], 20480)
    assert q.shape == (2, 22)
    _hold(y, q, x.numpy(), [300, -300], "b = 2, W = 20480")


def test_sines_constants_and_zeros_tie_as_the_statement_ties():
    t = np.arange(W) / 16000.0
    rows = [0.5 * np.sin(2 * np.pi * 440.0 * t), 0.5 * np.sin(2 * np.pi * 440.0 * t), 0.3 * np.sin(2 * np.pi * 1000.0 * t),
            0.3 * np.sin(2 * np.pi * 125.0 * t), np.full(W, 0.25), np.full(W, -0.7), np.zeros(W), np.zeros(W)]
    x = np.stack(rows).astype(np.float32)
    cents = [300, -300, 57, -1, 100, -1200, 1200, -57]
    y, q = _shift(torch.from_numpy(x).to(DEV), cents, W)
    _hold(y, q, x, cents, "sines, constants, zeros")
    host = PO.tables(cents, W)
    q = q.cpu().numpy()
    for i in (6, 7):                                           # all zero: every cost ties at 0, the first candidate wins
        assert not y[i].any() and np.array_equal(q[i, 1:], host["nominal"][i, 1:] - PO.R // 2)
    # a constant: the first segment's candidates (all inside the window for +100 cents) tie too
    assert q[4, 1] == host["nominal"][4, 1] - PO.R // 2


# ----------------------------------------------------------------------------- packs, batches, launches
def test_nothing_outside_the_window_is_read_and_a_row_does_not_depend_on_its_batch():
    cents = [300, -300, 57, -1200, 1200, 0]
    b = len(cents)
    x = _speechlike(b, W, 31)
    y, q = _shift(x.to(DEV), cents, W)
    # the same windows inside a pack whose every other sample is 1e30: before the first, between them, behind the last
    gap = 777
    pack = torch.full((b * (W + gap) + gap,), 1e30)
    offsets = [gap + i * (W + gap) for i in range(b)]
    for i, o in enumerate(offsets):
        pack[o:o + W] = x[i]
    flat = da.FlatWindows(pack.to(DEV), torch.tensor(offsets, dtype=torch.int64, device=DEV))
    y_flat, q_flat = _shift(flat, cents, W)
    assert torch.equal(y_flat, y) and torch.equal(q_flat, q)
    # windows that touch each other, in another order
    touching = da.FlatWindows(x.reshape(-1).to(DEV), torch.tensor([W * i for i in reversed(range(b))], dtype=torch.int64, device=DEV))
    y_rev, q_rev = _shift(touching, list(reversed(cents)), W)
    assert torch.equal(y_rev.flip(0), y) and torch.equal(q_rev.flip(0), q)
    # a window that leaves the vector reads zeros there: the last 500 samples of the pack and nothing behind them
    tail = da.FlatWindows(x[0].to(DEV), torch.tensor([W - 500, -300], dtype=torch.int64, device=DEV))
    cut = np.zeros((2, W), np.float32)
    cut[0, :500], cut[1, 300:] = x[0, W - 500:].numpy(), x[0, :W - 300].numpy()
    y_tail, q_tail = _shift(tail, [200, -200], W)
    _hold(y_tail, q_tail, cut, [200, -200], "windows that leave the vector")
    # every row alone (its own, smaller table of starts): the same bits
    for i, c in enumerate(cents):
        y1, q1 = _shift(x[i:i + 1].to(DEV), [c], W)
        assert torch.equal(y1[0], y[i]) and torch.equal(q1[0], q[i, :q1.shape[1]]), i
    # a second launch: the same bits
    y2, q2 = _shift(x.to(DEV), cents, W)
    assert torch.equal(y2, y) and torch.equal(q2, q)


def test_outputs_are_fully_overwritten_and_nothing_beyond_them_is_written():
    b, guard = 5, 1024
    for w in (2048, 1313, 1):
        cents = [1200, -1200, 0, 300, -57]
        x = _speechlike(b, w, 41).to(DEV)
        _host, tables = _tables(cents, w)
        J = tables["nominal"].shape[1]
        ybuf = torch.full((guard + b * w + guard,), float("nan"), device=DEV)
        qbuf = torch.full((guard + b * J + guard,), Q_FILL, dtype=torch.int32, device=DEV)
        out, q = ybuf[guard:guard + b * w].view(b, w), qbuf[guard:guard + b * J].view(b, J)
        assert _entry(x, tables, out, q, b, w) == 0
        torch.cuda.synchronize()
        assert torch.isfinite(out).all() and not (q == Q_FILL).any()
        assert torch.isnan(ybuf[:guard]).all() and torch.isnan(ybuf[guard + b * w:]).all()
        assert (qbuf[:guard] == Q_FILL).all() and (qbuf[guard + b * J:] == Q_FILL).all()
        _hold(out, q, x.cpu().numpy(), cents, f"guarded buffers, W = {w}")


def test_every_refusal_leaves_the_outputs_untouched():
    lib = _lib.load()
    b = 3
    x = _speechlike(b, W, 51).to(DEV)
    _host, tables = _tables([100, -100, 0], W)
    out = torch.full((b, W), float("nan"), device=DEV)
    q = torch.full((b, tables["nominal"].shape[1]), Q_FILL, dtype=torch.int32, device=DEV)

    def refused(status, word):
        torch.cuda.synchronize()
        assert status == -1 and word.encode() in lib.cpc_last_error(), (status, lib.cpc_last_error())
        assert torch.isnan(out).all() and (q == Q_FILL).all()

    refused(_entry(x, tables, out, q, b, 0), "augment_pitch")
    refused(_entry(x, tables, out, q, b, -5), "augment_pitch")
    refused(_entry(x, tables, out, q, b, W, segments=0), "augment_pitch")
    refused(_entry(x, tables, out, q, b, W, segments=-1), "augment_pitch")
    refused(_entry(x, tables, out, q, b, W, bound=1201), "1200")
    refused(_entry(x, tables, out, q, b, W, bound=-1), "1200")
    refused(_entry(x, tables, out, q, -1, W), "augment_pitch")
    refused(_entry(None, tables, out, q, b, W), "null pointer")
    for missing in ("ratio", "cutoff", "cents", "nominal"):
        holed = dict(tables)
        holed[missing] = None
        refused(_entry(x, holed, out, q, b, W, segments=tables["nominal"].shape[1], bound=100), "null pointer")
    refused(_entry(x, tables, None, q, b, W), "null pointer")
    refused(_entry(x, tables, out, None, b, W), "null pointer")
    offsets = torch.zeros(b, dtype=torch.int64, device=DEV)                                # offsets without the vector's length
    refused(_entry(x, tables, out, q, b, W, operand=(ptr(x), 0, ptr(offsets))), "vector's length")
    same = x.clone()
    assert _entry(same, tables, same, q, b, W) == -1 and b"must not be the input" in lib.cpc_last_error()
    assert torch.equal(same, x) and (q == Q_FILL).all()
    # b == 0: nothing to do, nothing done -- with or without pointers
    assert _entry(x, tables, out, q, 0, W) == 0 and _entry(None, tables, None, None, 0, W) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and (q == Q_FILL).all()
    with pytest.raises(ValueError, match="at most 1200"):
        audio.pitch_shift(x, 1201)


# ----------------------------------------------------------------------------- the transform and the direct call
def test_the_transform_and_the_direct_call_replay_their_plan():
    np.random.seed(61)
    aug = da.PitchShiftAugment(300)
    x = _speechlike(6, W, 62).to(DEV)
    kept = x.clone()
    y = aug(x.view(6, 1, W))
    assert y.shape == (6, 1, W) and torch.equal(x, kept)
    plan, starts = aug.last_plan, aug.last_offsets
    np.random.seed(61)
    assert plan["cents"].tolist() == [int(np.random.randint(-300, 300)) for _ in range(6)] and plan["window"] == W
    _hold(y.view(6, W), starts, kept.cpu().numpy(), plan["cents"].tolist(), "transform on a batch")
    assert torch.equal(aug.apply(plan, 0, 6, kept.clone()), y.view(6, W))             # the same plan again: the same bits
    assert torch.equal(aug.last_offsets, starts) and aug.last_offsets is not starts
    part = aug.apply(plan, 2, 5, kept[2:5].contiguous())                              # rows of a plan
    assert torch.equal(part, y.view(6, W)[2:5])
    with pytest.raises(ValueError, match="sealed for windows of 2048"):
        aug.apply(plan, 0, 6, _speechlike(6, 1024, 1).to(DEV))
    # pitch_wsola then time_dropout, the stand-in for the reference's pitch_dropout: the span is zero, the rest is the shift's
    np.random.seed(63)
    both = da.CombinedTransforms(["pitch_wsola", "time_dropout"], shift_max=300, t_ms=20)
    z = both(kept.view(6, 1, W)).view(6, W)
    shift, drop = both.last_plan["parts"]
    alone = aug.apply(shift, 0, 6, kept.clone())
    for i in range(6):
        s, n = int(drop["start"][i]), int(drop["length"][i])
        assert not z[i, s:s + n].any() and torch.equal(z[i, :s], alone[i, :s]) and torch.equal(z[i, s + n:], alone[i, s + n:])
    # the direct call: one int for all rows, one value per row, any leading shape
    one = audio.pitch_shift(kept.view(2, 3, W), 57)
    assert one.shape == (2, 3, W) and torch.equal(one.view(6, W), _shift(kept, [57] * 6, W)[0])
    rows, q = audio.pitch_shift(kept, plan["cents"], return_offsets=True)
    assert torch.equal(rows, y.view(6, W)) and torch.equal(q, starts)
    assert torch.equal(audio.pitch_shift(kept, 0), kept)
    with pytest.raises(ValueError, match="5 values of cents for 6 rows"):
        audio.pitch_shift(kept, [1, 2, 3, 4, 5])
    with pytest.raises(TypeError, match="whole numbers"):
        audio.pitch_shift(kept, 1.5)


# ----------------------------------------------------------------------------- the feeder and the command line
def _seed(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def test_feeder_yields_the_replay_of_the_plan_it_drew(capsys):
    w = 20480
    _seed(71)
    aug = da.PitchShiftAugment(300)
    seqs, speakers = ds.findAllSeqs(DB, extension=".flac")
    seqs = sorted(seqs, key=lambda s: s[1])
    speech = ds.AudioBatchData(DB, w, seqs, None, len(speakers), device=DEV, augmentation=aug, augment_past=True)
    loader = speech.getDataLoader(8, "samespeaker", True)
    out = [(s.clone(), l.clone()) for s, l in loader]
    pack, = loader.plans
    assert pack["future"] is None and pack["past"]["kind"] == "pitch_wsola" and len(out) == len(pack["batches"]) > 2
    np.random.seed(71)
    flat = speech.data.cpu()
    row = 0
    for i, ((seq, _label), offsets) in enumerate(zip(out, pack["batches"])):
        b = len(offsets)
        clean = torch.stack([flat[o:o + w] for o in offsets])
        assert seq.shape == (b, 2, 1, w) and torch.equal(seq[:, 1, 0].cpu(), clean)      # the future half stays clean
        if i < 2:                                                                       # (the replay costs 0.04 s per window)
            want, _q, bound = PO.replay(pack["past"], clean.numpy(), row, row + b)
            err = np.abs(seq[:, 0, 0].double().cpu().numpy() - want)
            assert (err <= bound).all(), f"batch {i}: worst error / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}"
            assert any(c != 0 for c in pack["past"]["cents"][row:row + b])
        row += b
    assert row == pack["past"]["n"] and -300 <= pack["past"]["cents"].min() and pack["past"]["cents"].max() < 300


def test_main_trains_with_pitch_wsola_and_time_dropout(tmp_path, monkeypatch, capsys):
    seen = []
    original = ds.AudioBatchData.augmented_from

    def watched(self, *a, **k):
        seen.append([type(t).__name__ for t in self.augmentation.transfors_cfgs])
        return original(self, *a, **k)

    monkeypatch.setattr(ds.AudioBatchData, "augmented_from", watched)
    run_dir = str(tmp_path / "pitch")
    os.makedirs(run_dir)
    argv = ["--pathDB", DB, "--pathCheckpoint", os.path.join(run_dir, "run"), "--path_cache", os.path.join(run_dir, "seqs_cache.txt"),
            "--hiddenEncoder", "64", "--hiddenGar", "64", "--nPredicts", "4", "--negativeSamplingExt", "16", "--arMode", "GRU",
            "--rnnMode", "linear", "--batchSizeGPU", "8", "--nGPU", "1", "--random_seed", "0", "--save_step", "1",
            "--pathTrain", SEQ_LIST, "--pathVal", SEQ_LIST, "--nEpoch", "1",
            "--augment_past", "--augment_type", "pitch_wsola", "time_dropout", "--shift_max", "300"]
    res = tr.main(argv)
    assert res.logs["epoch"] == [0] and len(seen) >= 2 and seen[0] == ["PitchShiftAugment", "TimeDropoutAugment"]
    for key in ("locLoss_train", "locLoss_val"):
        assert len(res.logs[key]) == 1 and np.isfinite(np.asarray(res.logs[key], dtype=np.float64)).all(), key
    with open(os.path.join(run_dir, "run", "checkpoint_args.json")) as fh:
        written = json.load(fh)
    assert written["augment_type"] == ["pitch_wsola", "time_dropout"] and written["augment_past"] is True and written["shift_max"] == 300
