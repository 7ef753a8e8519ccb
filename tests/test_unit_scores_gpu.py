"""cpc_unit_counts / cpc_unit_boundaries (csrc/unit_scores.hip), cpc2_amd.unit_scores and the unit_quality tool on the GPU against
unit_scores_oracle.py.  Every device output is an integer and is compared with ==.  The raw entry points run in poisoned buffers:
the packs' gaps and the frames behind an utterance's compared length hold out-of-range garbage, the scratch is 0xFF, and guard
words of 0xFF sit before and behind every output."""
import json

import numpy as np
import pytest
import torch

import unit_scores_oracle as UO
from cpc2_amd import _lib
from cpc2_amd import unit_scores as us
from cpc2_amd._lib import ptr, stream_ptr
from cpc2_amd.clustering.clustering import kmeans_assign
from cpc2_amd.eval import unit_quality as uq

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD = 16
GARBAGE = (-7, 0x7FFFFFF0, -(2 ** 31), 1 << 20)
LDS, GLOBAL, PLAIN, FOLD = 1, 2, 4, 8
LIB = _lib.load()
CELLS, CHUNK = LIB.cpc_unit_counts_lds_cells(), LIB.cpc_unit_counts_chunk()


def expected_form(n_units, n_phones):
    """The selection predicate of cpc_unit_counts(form = 0), restated: the table lives in LDS when it has at most CELLS cells."""
    return "lds" if n_units * n_phones <= CELLS else "global"


class Guarded:
    """n elements of `dtype` on the device between two runs of GUARD 0xFF elements; the payload zeroed or 0xFF."""

    def __init__(self, n, dtype, zero):
        self.n, self.size = n, torch.empty(0, dtype=dtype).element_size()
        raw = torch.full(((n + 2 * GUARD) * self.size,), 0xFF, dtype=torch.uint8, device=DEV)
        self.all = raw.view(dtype)
        self.body = self.all[GUARD:GUARD + n]
        if zero:
            self.body.zero_()

    def ptr(self):
        return ptr(self.all[GUARD:]) if self.n else ptr(self.all[GUARD:GUARD + 1])

    def read(self):
        """The payload on the host; asserts the guards."""
        host = self.all.cpu().numpy()
        edges = np.concatenate([host[:GUARD], host[GUARD + self.n:]])
        assert (np.ascontiguousarray(edges).view(np.uint8) == 0xFF).all(), "a guard word was written"
        return host[GUARD:GUARD + self.n].copy()

    def untouched(self):
        return (np.ascontiguousarray(self.all.cpu().numpy()).view(np.uint8) == 0xFF).all()


def pack(seqs, order=None, gap=3):
    """The sequences laid out in `order` with `gap` garbage words before, between and behind them -> (flat int32, offsets int64 by
    sequence index)."""
    order = list(range(len(seqs))) if order is None else order
    total = gap + sum(len(seqs[i]) + gap for i in order)
    flat = np.array([GARBAGE[j % len(GARBAGE)] for j in range(total)], dtype=np.int64).astype(np.int32)
    offsets = np.zeros(len(seqs), np.int64)
    at = gap
    for i in order:
        offsets[i] = at
        flat[at:at + len(seqs[i])] = seqs[i]
        at += len(seqs[i]) + gap
    return flat, offsets


def _tail(seq, extra):
    """seq followed by `extra` garbage frames: what lies behind the compared length is never read."""
    return np.concatenate([np.asarray(seq, dtype=np.int64), np.array(GARBAGE[:extra], dtype=np.int64)]).astype(np.int32)


class Batch:
    """Utterances (units[i], labels[i] cut to the compared length; labels None: the NULL form) packed with garbage for the ABI."""

    def __init__(self, units, labels, order=None, gap=3):
        self.units, self.labels = [np.asarray(z, dtype=np.int64) for z in units], labels
        self.want = {}                                                 # the oracle's tables by (n_units, n_phones): made once
        u = len(units)
        rev = None if order is None else order[::-1]
        tails = 1 if gap else 0                                        # gap 0: the utterances touch in the packs
        flat_u, off_u = pack([_tail(z, tails * (1 + i % 2)) for i, z in enumerate(units)], order, gap)
        self.du, self.dou = torch.from_numpy(flat_u).to(DEV), torch.from_numpy(off_u).to(DEV)
        self.dl = self.dol = None
        if labels is not None:
            flat_l, off_l = pack([_tail(y, tails * (i % 3)) for i, y in enumerate(labels)], rev, 2 * gap)   # (another layout than the units')
            self.dl, self.dol = torch.from_numpy(flat_l).to(DEV), torch.from_numpy(off_l).to(DEV)
        self.lengths = np.array([len(z) for z in units], dtype=np.int32)
        self.dlen = torch.from_numpy(self.lengths).to(DEV) if u else torch.zeros(1, dtype=torch.int32, device=DEV)
        self.u = u

    def args(self):
        return (ptr(self.du), self.du.numel(), ptr(self.dou), ptr(self.dl), 0 if self.dl is None else self.dl.numel(), ptr(self.dol),
                ptr(self.dlen), self.u)


def run_counts(batch, n_units, n_phones, form=0, tables=None):
    """cpc_unit_counts through the raw ABI -> (joint, unit_runs, phone_runs, invalid) on the host; `tables`: Guarded outputs of an
    earlier call, added to."""
    if tables is None:
        tables = (Guarded(n_units * n_phones, torch.int64, True), Guarded(n_units, torch.int64, True),
                  Guarded(n_phones, torch.int64, True), Guarded(1, torch.int64, True))
    need = LIB.cpc_unit_counts_scratch_bytes(batch.u)
    scratch = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device=DEV)
    status = LIB.cpc_unit_counts(*batch.args(), n_units, n_phones, form, *[t.ptr() for t in tables], ptr(scratch), need, stream_ptr(DEV))
    assert status == 0, LIB.cpc_last_error()
    torch.cuda.synchronize()
    assert (scratch[need:].cpu().numpy() == 0xFF).all()
    joint, unit_runs, phone_runs, invalid = (t.read() for t in tables)
    return (joint.reshape(n_units, n_phones), unit_runs, phone_runs, int(invalid[0])), tables


def assert_counts(batch, n_units, n_phones, form=0):
    got, _ = run_counts(batch, n_units, n_phones, form)
    if (n_units, n_phones) not in batch.want:
        batch.want[n_units, n_phones] = UO.tables(batch.units, batch.labels, n_units, n_phones)
    want = batch.want[n_units, n_phones]
    for g, w, name in zip(got, want, ("joint", "unit_runs", "phone_runs", "invalid")):
        assert np.array_equal(g, w), (name, np.argwhere(np.asarray(g) != np.asarray(w))[:5])
    return got


def run_boundaries(batch, tol, out=None, total=None):
    total = int(batch.lengths.sum()) if total is None else total
    out = Guarded(batch.u * 5, torch.int32, False) if out is None else out
    need = LIB.cpc_unit_boundaries_scratch_bytes(batch.u, total)
    scratch = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device=DEV)
    status = LIB.cpc_unit_boundaries(*batch.args(), total, tol, out.ptr(), ptr(scratch), need, stream_ptr(DEV))
    assert status == 0, LIB.cpc_last_error()
    torch.cuda.synchronize()
    assert (scratch[need:].cpu().numpy() == 0xFF).all()
    return out.read().reshape(batch.u, 5), out


def runs(rs, n, n_symbols, mean_run):
    """n symbols in runs of geometric length."""
    out = np.zeros(n, np.int64)
    f = 0
    while f < n:
        k = int(rs.geometric(1.0 / mean_run))
        out[f:f + k] = rs.randint(n_symbols)
        f += k
    return out


def random_batch(seed, lengths, n_units, n_phones, with_labels=True, order=None):
    rs = np.random.RandomState(seed)
    units = [runs(rs, n, n_units, 3) for n in lengths]
    labels = [runs(rs, n, n_phones, 8) for n in lengths] if with_labels else None
    return Batch(units, labels, order)


# ----------------------------------------------------------------------------- smallest shapes
@pytest.mark.parametrize("length", [0, 1, 2])
def test_one_utterance_of_length(length):
    batch = Batch([[2, 1][:length]], [[0, 3][:length]])
    got = assert_counts(batch, 3, 4)
    assert got[0].sum() == length and got[1].sum() == length
    rows, _ = run_boundaries(batch, 2)
    assert rows.tolist() == [[1, 1, 1, 1, 1] if length == 2 else [0] * 5]


def test_no_utterance_is_a_no_op():
    tables = [Guarded(3, torch.int64, False), Guarded(3, torch.int64, False), Guarded(1, torch.int64, False), Guarded(1, torch.int64, False)]
    assert LIB.cpc_unit_counts(None, 0, None, None, 0, None, None, 0, 3, 1, 0, *[t.ptr() for t in tables], None, 0, stream_ptr(DEV)) == 0
    out = Guarded(5, torch.int32, False)
    assert LIB.cpc_unit_boundaries(None, 0, None, None, 0, None, None, 0, 0, 2, out.ptr(), None, 0, stream_ptr(DEV)) == 0
    torch.cuda.synchronize()
    assert all(t.untouched() for t in tables) and out.untouched()
    empty = us.count(torch.zeros(1, dtype=torch.int32, device=DEV), None, torch.zeros(0, dtype=torch.int64), None,
                     torch.zeros(0, dtype=torch.int32), 3, 1)
    assert int(empty.joint.sum()) == 0 and empty.boundaries.shape == (0, 5)


def test_labels_null():
    batch = random_batch(1, [40, 1, 0, 700], 9, 1, with_labels=False)
    got = assert_counts(batch, 9, 1)
    assert got[2].tolist() == [3]                                      # one run of label 0 per non-empty utterance
    rows, _ = run_boundaries(batch, 2)
    want = [UO.boundaries(z, None, 2) for z in batch.units]
    assert rows.tolist() == want and all(r[0] == 0 and r[2:] == [0, 0, 0] for r in want)


# ----------------------------------------------------------------------------- both table forms at their edge
SHAPES = [(512, 32, "lds"), (513, 32, "global"), (16384, 1, "lds"), (1, 1024, "lds"), (2000, 41, "global"), (50, 41, "lds"),
          (16384, 1024, "global")]


@pytest.mark.parametrize("n_units,n_phones,form", SHAPES, ids=[f"{u}x{p}-{f}" for u, p, f in SHAPES])
def test_table_forms(n_units, n_phones, form):
    assert expected_form(n_units, n_phones) == form
    assert (512 * 32 == CELLS) and 513 * 32 > CELLS                   # the first two shapes ARE the limit and one row beyond it
    lengths = [CHUNK + 37, 900, 0, 1, 2500, 64, 63, 65, 3001]
    batch = random_batch(n_units + n_phones, lengths, n_units, n_phones, order=[3, 0, 8, 1, 6, 2, 7, 5, 4])
    rs = np.random.RandomState(5)
    for z, y in zip(batch.units, batch.labels):                        # the corners of the table are hit
        if len(z) > 10:
            z[rs.randint(len(z))], y[rs.randint(len(y))] = n_units - 1, n_phones - 1
    batch = Batch(batch.units, batch.labels, order=[3, 0, 8, 1, 6, 2, 7, 5, 4])
    auto = assert_counts(batch, n_units, n_phones, 0)
    if n_units * n_phones <= 1 << 20:                                  # (the 128 MB table goes through once)
        forced = assert_counts(batch, n_units, n_phones, GLOBAL)       # the global form takes every shape
        assert all(np.array_equal(a, b) for a, b in zip(auto, forced))
        assert_counts(batch, n_units, n_phones, GLOBAL | PLAIN)
    if form == "lds":
        assert_counts(batch, n_units, n_phones, LDS)
        assert_counts(batch, n_units, n_phones, LDS | FOLD)
    else:
        tables = [Guarded(8, torch.int64, False) for _ in range(4)]
        need = LIB.cpc_unit_counts_scratch_bytes(batch.u)
        scratch = torch.zeros(need, dtype=torch.uint8, device=DEV)
        assert LIB.cpc_unit_counts(*batch.args(), n_units, n_phones, LDS, *[t.ptr() for t in tables], ptr(scratch), need,
                                   stream_ptr(DEV)) == -1 and b"form=1" in LIB.cpc_last_error()
        assert all(t.untouched() for t in tables)


# ----------------------------------------------------------------------------- one hot cell
@pytest.mark.parametrize("form", [LDS, GLOBAL, LDS | FOLD, GLOBAL | PLAIN], ids=["lds", "global", "lds-folded", "global-plain"])
def test_one_hot_cell(form):
    n = 1 << 20
    zeros = torch.zeros(n + 8, dtype=torch.int32, device=DEV)
    off = torch.tensor([3], dtype=torch.int64, device=DEV)
    length = torch.tensor([n], dtype=torch.int32, device=DEV)
    tables = (Guarded(12, torch.int64, True), Guarded(4, torch.int64, True), Guarded(3, torch.int64, True), Guarded(1, torch.int64, True))
    need = LIB.cpc_unit_counts_scratch_bytes(1)
    scratch = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    assert LIB.cpc_unit_counts(ptr(zeros), n + 8, ptr(off), ptr(zeros), n + 8, ptr(off), ptr(length), 1, 4, 3, form,
                               *[t.ptr() for t in tables], ptr(scratch), need, stream_ptr(DEV)) == 0, LIB.cpc_last_error()
    torch.cuda.synchronize()
    joint, unit_runs, phone_runs, invalid = (t.read() for t in tables)
    assert joint.tolist() == [n] + [0] * 11 and unit_runs.tolist() == [1, 0, 0, 0] and phone_runs.tolist() == [1, 0, 0]
    assert invalid.tolist() == [0]


# ----------------------------------------------------------------------------- chunk edges
@pytest.mark.parametrize("form", [0, GLOBAL], ids=["lds", "global"])
def test_chunk_edges(form):
    for first in (CHUNK - 1, CHUNK, CHUNK + 1):
        rs = np.random.RandomState(first)
        z, y = runs(rs, first + 300, 7, 3), runs(rs, first + 300, 5, 8)
        z[CHUNK - 4:CHUNK + 4] = 6                                     # a run across the chunk edge of the flat frame space
        y[CHUNK - 9:CHUNK + 2] = 4
        one = Batch([z[:first]], [y[:first]])
        assert_counts(one, 7, 5, form)
        # the next utterance starts with the unit and the label the first one ends with: two runs, not one
        nxt_z, nxt_y = np.concatenate([[z[first - 1]] * 3, z[first:]]), np.concatenate([[y[first - 1]] * 2, y[first - 1:first + 300]])[:303]
        two = Batch([z[:first], nxt_z, z[:5]], [y[:first], nxt_y, y[:5]], gap=0)
        got = assert_counts(two, 7, 5, form)
        alone = UO.tables([z[:first]], [y[:first]], 7, 5)
        assert got[1].sum() > alone[1].sum() + 1
        # permuted order, gaps between the utterances
        assert_counts(Batch([z[:first], nxt_z, z[:5], z[:0], nxt_z[:1]], [y[:first], nxt_y, y[:5], y[:0], nxt_y[:1]],
                            order=[2, 4, 1, 3, 0], gap=11), 7, 5, form)


def test_runs_do_not_merge_across_utterances():
    batch = Batch([[3, 3, 3], [3, 3], [3]], [[1, 1, 1], [1, 1], [1]], gap=0)     # adjacent in the pack, equal symbols
    got = assert_counts(batch, 4, 2)
    assert got[1].tolist() == [0, 0, 0, 3] and got[2].tolist() == [0, 3] and got[0][3, 1] == 6


# ----------------------------------------------------------------------------- accumulation / overwriting
def test_two_halves_with_into_equal_the_whole():
    lengths = [300, 0, 1200, 5, 77, 4100, 2]
    whole = random_batch(11, lengths, 60, 12)

    def dev(batch, rows):
        z = [batch.units[i] for i in rows]
        y = [batch.labels[i] for i in rows]
        zo = np.concatenate([[0], np.cumsum([len(a) for a in z][:-1])]).astype(np.int64)
        return (torch.from_numpy(np.concatenate(z).astype(np.int32)).to(DEV), torch.from_numpy(np.concatenate(y).astype(np.int32)).to(DEV),
                torch.from_numpy(zo).to(DEV), torch.from_numpy(zo).to(DEV), torch.tensor([len(a) for a in z], dtype=torch.int32, device=DEV))

    all_rows = list(range(len(lengths)))
    once = us.count(*dev(whole, all_rows), 60, 12, tol=1)
    first = us.count(*dev(whole, all_rows[:3]), 60, 12, tol=1)
    both = us.count(*dev(whole, all_rows[3:]), 60, 12, tol=1, into=first)
    assert both.joint.data_ptr() == first.joint.data_ptr()            # (added in place: `first` is spent)
    for a, b in zip(once[:4], both[:4]):
        assert torch.equal(a, b)
    assert np.array_equal(once.boundaries, both.boundaries) and once.boundaries.shape == (7, 5)
    want = UO.tables(whole.units, whole.labels, 60, 12)
    assert np.array_equal(once.joint.cpu().numpy(), want[0]) and np.array_equal(once.unit_runs.cpu().numpy(), want[1])
    assert np.array_equal(once.phone_runs.cpu().numpy(), want[2]) and int(once.invalid) == 0
    assert once.boundaries.tolist() == [UO.boundaries(z, y, 1) for z, y in zip(whole.units, whole.labels)]
    with pytest.raises(ValueError, match="into"):
        us.count(*dev(whole, all_rows[3:]), 60, 12, tol=2, into=both)
    # the raw entry adds: a second call on the same tables doubles them
    _, tables = run_counts(whole, 60, 12)
    twice, _ = run_counts(whole, 60, 12, tables=tables)
    assert np.array_equal(twice[0], 2 * want[0]) and np.array_equal(twice[1], 2 * want[1]) and np.array_equal(twice[2], 2 * want[2])


def test_boundaries_overwrite():
    batch = random_batch(12, [500, 3, 0, 64, 65], 9, 6)
    rows, out = run_boundaries(batch, 2)
    again, _ = run_boundaries(batch, 2, out=out)                       # into what the first call left
    assert np.array_equal(rows, again)
    assert rows.tolist() == [UO.boundaries(z, y, 2) for z, y in zip(batch.units, batch.labels)]


# ----------------------------------------------------------------------------- invalid ids
def test_invalid_ids_are_counted_and_never_used_as_an_index():
    n_units, n_phones = 6, 4
    batch = random_batch(13, [200, 90, 300], n_units, n_phones)
    batch.units[1][17], batch.units[1][60], batch.labels[2][5] = -1, n_units, n_phones
    batch = Batch(batch.units, batch.labels)
    for form in (LDS, GLOBAL):
        got = assert_counts(batch, n_units, n_phones, form)            # (the oracle leaves those frames out of every table)
        assert got[3] == 3 and got[0].sum() == 590 - 3
    lengths = torch.from_numpy(batch.lengths).to(DEV)
    with pytest.raises(ValueError, match=r"3 invalid frames; utterance 1 is the first: frame 17 has unit -1"):
        us.count(batch.du, batch.dl, batch.dou, batch.dol, lengths, n_units, n_phones)
    # an utterance that leaves its pack is not read: its frames are invalid, the others are counted
    off = batch.dou.clone()
    off[2] = batch.du.numel() - 100
    moved = Batch(batch.units, batch.labels)
    moved.dou = off
    got, _ = run_counts(moved, n_units, n_phones)
    want = UO.tables(batch.units[:2], batch.labels[:2], n_units, n_phones)
    assert np.array_equal(got[0], want[0]) and got[3] == want[3] + 300
    rows, _ = run_boundaries(moved, 2)
    assert rows[2].tolist() == [-1] * 5 and rows[0].tolist() == UO.boundaries(batch.units[0], batch.labels[0], 2)


# ----------------------------------------------------------------------------- boundaries
@pytest.mark.parametrize("tol", [0, 1, 2, 5])
def test_boundaries_against_the_oracle(tol):
    rs = np.random.RandomState(20 + tol)
    lengths = [700, 64, 65, 66, 129, 2, 1, 0, 3000]
    units = [runs(rs, n, 12, 3) for n in lengths]
    labels = [runs(rs, n, 9, 8) for n in lengths]
    units += [runs(rs, 150, 5, 3), np.full(150, 4), np.arange(150) % 7, np.arange(200) % 2]
    labels += [np.full(150, 2), runs(rs, 150, 5, 6), np.arange(150) % 5, runs(rs, 200, 6, 40)]   # no reference; no hypothesis; all change
    batch = Batch(units, labels, order=list(rs.permutation(len(units))))
    rows, _ = run_boundaries(batch, tol)
    want = [UO.boundaries(z, y, tol) for z, y in zip(batch.units, batch.labels)]
    assert rows.tolist() == want
    assert want[-4][0] == 0 and want[-3][1] == 0 and want[-2][:2] == [149, 149] and want[0][2] > 0
    short, _ = run_boundaries(batch, tol, total=int(batch.lengths.sum()) - 1)        # the lists of the last utterance do not fit
    assert (short == -1).all(axis=1).sum() == 1 and ((short == np.array(want)) | (short == -1)).all()


# ----------------------------------------------------------------------------- the --clustering path at function level
def test_assign_then_count():
    """Features = centroid + noise.  Distinct centroids are >= 4 apart in some coordinate (integer grid points scaled by 4) and the noise is
    below 0.5 per coordinate in 16 dimensions: the squared distance to the own centroid is < 16 * 0.25 = 4, to any other centroid
    > (4 - 0.5)^2 = 12.25: the margin 8.25 is five orders of magnitude above any float32 doubt at these magnitudes (values <= 32,
    squares <= 1024, eps 6e-8 * 16 terms * 1024 = 1e-3)."""
    rs = np.random.RandomState(30)
    k, d, lengths = 24, 16, [400, 37, 1, 900]
    centroids = (4.0 * rs.randint(0, 8, size=(k, d))).astype(np.float32)
    units = [runs(rs, n, k, 3) for n in lengths]
    flat = np.concatenate(units)
    noise = (rs.rand(len(flat), d) - 0.5).astype(np.float32) * 0.98
    feats = centroids[flat] + noise
    d2 = ((feats[:, None, :].astype(np.float64) - centroids[None].astype(np.float64)) ** 2).sum(-1)
    own = d2[np.arange(len(flat)), flat]
    d2[np.arange(len(flat)), flat] = np.inf
    assert (d2.min(axis=1) - own).min() > 8.0                          # the stated margin, on every frame: no case is excluded
    index, _ = kmeans_assign(torch.from_numpy(feats).to(DEV), torch.from_numpy(centroids).to(DEV).view(1, k, d), want_min_sq=False)
    labels = [runs(rs, n, 7, 8) for n in lengths]
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths[:-1])]).astype(np.int64)).to(DEV)
    got = us.count(index, torch.from_numpy(np.concatenate(labels).astype(np.int32)).to(DEV), offsets, offsets,
                   torch.tensor(lengths, dtype=torch.int32, device=DEV), k, 7)
    want = UO.tables(units, labels, k, 7)
    assert np.array_equal(got.joint.cpu().numpy(), want[0]) and np.array_equal(got.unit_runs.cpu().numpy(), want[1])
    assert np.array_equal(got.phone_runs.cpu().numpy(), want[2])


# ----------------------------------------------------------------------------- the tool end to end
def test_tool_end_to_end(tmp_path):
    rs = np.random.RandomState(40)
    names = [f"spk{i % 3}-utt{i}" for i in range(9)]
    frames = [300, 41, 500, 7, 120, 64, 900, 33, 10]
    units = {n: runs(rs, f, 30, 3) for n, f in zip(names, frames)}
    shift = {names[1]: 2, names[2]: -1, names[4]: 5, names[6]: -2}                   # label lengths differ; names[4] by too much
    labels = {n: runs(rs, f + shift.get(n, 0), 11, 8) for n, f in zip(names, frames) if n != names[7]}      # names[7] has no labels
    quant, phone, out = tmp_path / "quantized_outputs.txt", tmp_path / "labels.txt", tmp_path / "out"
    quant.write_text("\n".join(f"some/dir/{n}.flac\t" + ",".join(str(v) for v in units[n]) for n in names))
    phone.write_text("".join(n + " " + " ".join(str(v) for v in labels[n]) + "\n" for n in labels))
    res = uq.main(["--quantized", str(quant), "--pathPhone", str(phone), "--out", str(out), "--tolerance", "1"])
    kept = [n for n in names if n not in (names[4], names[7])]
    assert res["names"] == kept and res["skipped"] == [names[7]] and [m["name"] for m in res["mismatched"]] == [names[4]]
    cut = {n: min(len(units[n]), len(labels[n])) for n in kept}
    zs, ys = [units[n][:cut[n]] for n in kept], [labels[n][:cut[n]] for n in kept]
    n_units, n_phones = max(int(v.max()) for v in units.values()) + 1, max(int(v.max()) for v in labels.values()) + 1
    joint, unit_runs, phone_runs, invalid = UO.tables(zs, ys, n_units, n_phones)
    assert invalid == 0
    saved = np.load(out / "joint_counts.npy")
    assert saved.dtype == np.int64 and np.array_equal(saved, joint)
    want, bound = UO.scores(joint, unit_runs, phone_runs, [UO.boundaries(z, y, 1) for z, y in zip(zs, ys)], 1, 0.01)
    report = json.loads((out / "unit_scores.json").read_text())
    UO.assert_scores_close(report["scores"], want, bound)
    assert report["n_utterances"] == 7 and report["n_frames"] == int(joint.sum()) and report["skipped"] == [names[7]]
    assert report["mismatched"] == [{"name": names[4], "frames": 120, "labels": 125}]
    assert report["unit_frames"] == joint.sum(axis=1).tolist() and report["phone_frames"] == joint.sum(axis=0).tolist()
    lines = (out / "unit_to_phone.txt").read_text().splitlines()
    assert [tuple(float(v) if "." in v else int(v) for v in ln.split()) for ln in lines] == UO.unit_to_phone(joint)
    with pytest.raises(ValueError, match="not an empty directory"):
        uq.main(["--quantized", str(quant), "--pathPhone", str(phone), "--out", str(out)])
    # without labels: the unit side only
    res = uq.main(["--quantized", str(quant), "--out", str(tmp_path / "plain")])
    want, bound = UO.scores(*UO.tables([units[n] for n in names], None, n_units, 1)[:3], has_labels=False)
    UO.assert_scores_close(res["scores"], want, bound)
    # nothing left to score
    phone.write_text("nobody 1 2 3\n")
    with pytest.raises(ValueError, match="no utterance left to score"):
        uq.main(["--quantized", str(quant), "--pathPhone", str(phone), "--out", str(tmp_path / "none")])


# ----------------------------------------------------------------------------- refusals of the C entries
def test_entry_points_refuse_before_any_launch():
    batch = random_batch(50, [30, 20], 5, 3)
    tables = [Guarded(15, torch.int64, False), Guarded(5, torch.int64, False), Guarded(3, torch.int64, False), Guarded(1, torch.int64, False)]
    out = Guarded(10, torch.int32, False)
    need = LIB.cpc_unit_boundaries_scratch_bytes(2, 50)
    scratch = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    a = list(batch.args())
    t = [x.ptr() for x in tables]

    def counts(args=a, n_units=5, n_phones=3, form=0, tabs=t, scr=ptr(scratch), size=need):
        return LIB.cpc_unit_counts(*args, n_units, n_phones, form, *tabs, scr, size, stream_ptr(DEV))

    def bounds(args=a, total=50, tol=2, o=out.ptr(), scr=ptr(scratch), size=need):
        return LIB.cpc_unit_boundaries(*args, total, tol, o, scr, size, stream_ptr(DEV))

    def swapped(i, value):
        return a[:i] + [value] + a[i + 1:]

    refused = [counts(args=swapped(0, None)), counts(args=swapped(2, None)), counts(args=swapped(5, None)), counts(args=swapped(6, None)),
               counts(tabs=[None] + t[1:]), counts(tabs=t[:1] + [None] + t[2:]), counts(tabs=t[:2] + [None] + t[3:]),
               counts(tabs=t[:3] + [None]), counts(scr=None), counts(args=swapped(7, -1)), counts(args=swapped(1, -1)),
               counts(args=swapped(4, -1)), counts(n_units=0), counts(n_units=16385), counts(n_phones=0), counts(n_phones=1025),
               counts(args=swapped(3, None), n_phones=3), counts(form=3), counts(form=12), counts(form=16), counts(form=-1),
               bounds(args=swapped(0, None)), bounds(args=swapped(2, None)), bounds(args=swapped(5, None)), bounds(args=swapped(6, None)),
               bounds(o=None), bounds(scr=None), bounds(args=swapped(7, -1)), bounds(total=-1), bounds(tol=-1)]
    assert refused == [-1] * len(refused), refused
    assert b"unit_boundaries" in LIB.cpc_last_error()
    assert counts(size=8) == -3 and bounds(size=need - 256) == -3      # CPC_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert all(x.untouched() for x in tables) and out.untouched()
    assert (scratch.cpu().numpy() == 0xFF).all()
