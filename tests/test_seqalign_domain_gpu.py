"""csrc/seqalign.hip across its accepted domain, through cpc2_amd.seq_alignment (beam_search_batch, align_score_batch), against
tests/per_oracle.py by EQUALITY: the search's scores as float32 bit patterns, label lists, sizes, counts, the tie flag and the
padding of every returned row; the alignment score as integers.  No tolerance anywhere: both kernels are exact.

Every search test first proves FROM THE ORACLE (per_oracle.beam_search's stats) that its input takes the path it is about -- a
group of equal scores that straddles the cut and is larger than the launch, the byte at which the radix select stops, a beam
that fills all nKeep * P slots, prefixes that re-enter the beam -- and only then compares.  All inputs are generated from seeds or
built in closed form; an oracle result is computed once per input and shared."""
import functools

import numpy as np
import pytest
import torch

import per_oracle
from cpc2_amd import seq_alignment as sa

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN = float("nan")


# --------------------------------------------------------------------------- helpers
def threads_of(n_keep, P):
    """The launch rule of cpc_ctc_beam_search (seqalign.hip): nKeep * P candidates -> 256 threads up to 2048 candidates, 512 up
    to 8192, 1024 above.  One pass of the kernel's loops over the candidates covers `threads` slots."""
    cand = n_keep * P
    return 256 if cand <= 2048 else (512 if cand <= 8192 else 1024)


def as_bits(out):
    return [(int(np.float32(s).view(np.uint32)), list(lab)) for s, lab in out]


def rows_of(scores, sizes, labels, counts, n):
    """Row n of a batch result as [(score bits, [labels])]; checks the padding (-1 behind the labels, 0 / 0 / -1 in the rows
    that hold no prefix) on the way."""
    scores, sizes, labels = scores[n].cpu().numpy(), sizes[n].cpu().numpy(), labels[n].cpu().numpy()
    kept = int(counts[n])
    assert 0 <= kept <= scores.shape[0]
    out = []
    for r in range(scores.shape[0]):
        if r < kept:
            assert 0 <= sizes[r] <= labels.shape[1]
            assert (labels[r, sizes[r]:] == -1).all() and (labels[r, :sizes[r]] >= 0).all()
            out.append((int(scores[r].view(np.uint32)), [int(x) for x in labels[r, :sizes[r]]]))
        else:
            assert scores[r].view(np.uint32) == 0 and sizes[r] == 0 and (labels[r] == -1).all()
    return out


class Oracle:
    """per_oracle.beam_search of one input with its stats."""

    def __init__(self, probs, n_keep, blank):
        self.stats = {}
        self.out, self.tie = per_oracle.beam_search(probs, n_keep, blank, stats=self.stats)
        self.want = as_bits(self.out)


def equals_oracle(res, n, oracle, best_only=False):
    """Row n of a beam_search_batch result against the oracle: every returned row, counts, the tie flag."""
    want = oracle.want[:1] if best_only else oracle.want
    assert res[0].dtype == torch.float32 and all(x.dtype == torch.int32 for x in res[1:])
    assert int(res[3][n]) == len(want)
    assert int(res[4][n]) == int(oracle.tie)
    got = rows_of(*res[:4], n)
    assert [len(lab) for _, lab in got] == [len(lab) for _, lab in want]
    assert got == want


def same_bytes(a, b):
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


def search(probs, lengths, n_keep, blank, best_only=False):
    probs = torch.as_tensor(probs)
    if probs.dim() == 2:
        probs = probs[None]
    if lengths is not None:
        lengths = torch.as_tensor(lengths).to(DEV)
    return sa.beam_search_batch(probs.to(DEV), lengths, n_keep, blank, best_only=best_only)


# --------------------------------------------------------------------------- 1. ties that straddle the cut
def level_rows(T, P, high, hi_exp, lo_exp):
    """T equal rows: the symbols in `high` at 2**-hi_exp, the others at 2**-lo_exp.  Powers of two: every product of the search
    is exact and non-zero, so equal scores are equal by arithmetic and not by accident."""
    row = np.full(P, 2.0 ** -lo_exp, np.float32)
    row[list(high)] = 2.0 ** -hi_exp
    return np.tile(row, (T, 1))


TIE_CASES = {
    # name: (probs, nKeep, blank)
    "uniform_1024thr": lambda: (level_rows(4, 128, [], 7, 7), 128, 77),
    "two_level_1024thr": lambda: (level_rows(3, 128, range(50, 90), 6, 8), 128, 77),
    "two_level_512thr": lambda: (level_rows(4, 64, range(20, 40), 5, 7), 100, 0),
    "two_level_256thr": lambda: (level_rows(4, 16, range(2, 10), 3, 5), 128, 9),
}


@functools.lru_cache(maxsize=None)
def tie_case(name):
    probs, n_keep, blank = TIE_CASES[name]()
    return probs, n_keep, blank, Oracle(probs, n_keep, blank)


@pytest.mark.parametrize("name", list(TIE_CASES))
def test_ties_that_straddle_the_cut_across_waves_and_passes(name):
    """More candidates at the cut score than the launch has threads, lying in more than one pass of `threads` slots: the tie
    placement loop counts across all waves (wave_count[]) and carries `placed` from pass to pass.  Twice: identical bytes."""
    probs, n_keep, blank, oracle = tie_case(name)
    P = probs.shape[1]
    threads = threads_of(n_keep, P)
    assert n_keep * P > threads and name.endswith(f"_{threads}thr")
    groups = oracle.stats["groups"]
    assert oracle.tie and groups
    big = [g for g in groups if g["size"] > threads and g["hi"] // threads > g["lo"] // threads]
    print(name, "threads", threads, "levels", oracle.stats["levels"], "groups", groups)
    assert big, groups
    assert all(0 < g["need"] < g["size"] for g in groups)
    a = search(probs, None, n_keep, blank)
    b = search(probs, None, n_keep, blank)
    same_bytes(a, b)
    equals_oracle(a, 0, oracle)


def test_some_tie_case_takes_its_members_from_a_later_pass_and_a_later_wave():
    """Over the cases above the LAST member that the beam takes of a straddling group lies beyond the first pass in one case (the
    count carried between passes decides its place) and beyond the first wave in another (the counts of the waves before)."""
    taken = []
    for name in TIE_CASES:
        probs, n_keep, _, oracle = tie_case(name)
        threads = threads_of(n_keep, probs.shape[1])
        taken += [(g["taken_hi"] // threads, (g["taken_hi"] % threads) // 64) for g in oracle.stats["groups"]]
    assert any(p > 0 for p, _ in taken) and any(w > 0 for _, w in taken), taken


# --------------------------------------------------------------------------- 2. every stop level of the select
STOP_SHIFTS = (22, 14, 7)


@functools.lru_cache(maxsize=None)
def stop_case(s):
    row = (2.0 ** -7 * (1 + np.arange(64) * 2.0 ** -s)).astype(np.float32)
    assert len(set(row.tolist())) == 64                       # exact in f32: 64 distinct values
    probs = np.tile(row, (2, 1))
    return probs, Oracle(probs, 10, 0)


def test_stop_cases_reach_every_level_of_the_select():
    levels = set()
    for s in STOP_SHIFTS:
        levels |= set(stop_case(s)[1].stats["levels"])
    assert levels == {0, 1, 2, 3}


@pytest.mark.parametrize("s", STOP_SHIFTS)
def test_select_stops_at_every_byte_without_ties(s):
    """Rows 2**-7 (1 + c 2**-s): the nKeep-th and the next score first differ in a byte that s chooses."""
    probs, oracle = stop_case(s)
    levels = oracle.stats["levels"]
    print("s", s, "levels", levels)
    assert levels and "tie" not in levels and not oracle.tie
    equals_oracle(search(probs, None, 10, 0), 0, oracle)


# --------------------------------------------------------------------------- 3. launch thresholds
LAUNCHES = [(128, 16), (121, 17), (128, 64), (127, 65), (128, 96), (128, 97)]       # (P, nKeep)


@functools.lru_cache(maxsize=None)
def launch_case(P, n_keep):
    g = torch.Generator().manual_seed(1000 * P + n_keep)
    probs = torch.softmax(2.0 * torch.randn(6, P, generator=g), 1).numpy()
    return probs, Oracle(probs, n_keep, P // 2)


def check_launch(P, n_keep):
    probs, oracle = launch_case(P, n_keep)
    assert oracle.stats["max_beam"] == n_keep                   # some frame used all nKeep * P slots
    assert not oracle.tie
    equals_oracle(search(probs, None, n_keep, P // 2), 0, oracle)


def test_launch_cases_sit_on_both_sides_of_every_threshold():
    assert [threads_of(k, P) for P, k in LAUNCHES] == [256, 512, 512, 1024, 1024, 1024]
    assert [4 * P * k > 48 * 1024 for P, k in LAUNCHES] == [False] * 5 + [True]      # dynamic LDS beyond 48 KiB: the opt-in
    assert 4 * 128 * 96 == 48 * 1024


@pytest.mark.parametrize("P,n_keep", LAUNCHES)
def test_launch_geometry_at_and_above_its_thresholds(P, n_keep):
    check_launch(P, n_keep)


def test_small_launch_then_opt_in_then_small_launch():
    """The launch that raises the kernel's dynamic LDS limit directly after a 256-thread launch, and a small one after it."""
    check_launch(128, 16)
    check_launch(128, 97)
    check_launch(128, 16)


# --------------------------------------------------------------------------- 4. long and ragged
def peaked(seed, T, P, conf, mean_run=6):
    """[T, P] probabilities that follow runs of one symbol (the blank P - 1 among them) at about `conf`."""
    g = torch.Generator().manual_seed(seed)
    n_runs = max(1, T // mean_run)
    cuts = sorted(torch.randperm(T - 1, generator=g)[:n_runs - 1].add(1).tolist()) if T > 1 else []
    bounds = [0] + cuts + [T]
    syms = torch.randint(0, P, (len(bounds) - 1,), generator=g)
    path = torch.empty(T, dtype=torch.long)
    for k in range(len(bounds) - 1):
        path[bounds[k]:bounds[k + 1]] = syms[k]
    logits = torch.randn(T, P, generator=g)
    logits[torch.arange(T), path] += float(np.log(conf / (1 - conf) * (P - 1)))
    return torch.softmax(logits, 1).numpy()


LONG_SEEDS = (11, 12, 13)
LONG_LENGTHS = (8192, 8000, 8192)
RAGGED_LENGTHS = (1, 2, 127, 128, 129, 1024)


@functools.lru_cache(maxsize=None)
def long_case(i):
    probs = peaked(LONG_SEEDS[i], 8192, 8, 0.999)
    return probs, Oracle(probs[:LONG_LENGTHS[i]], 4, 7)


@functools.lru_cache(maxsize=None)
def ragged_case(i):
    T = RAGGED_LENGTHS[i]
    probs = peaked(40 + i, T, 42, 0.99)
    return probs, Oracle(probs, 20, 41)


@functools.lru_cache(maxsize=None)
def underflow_case():
    g = torch.Generator().manual_seed(7)
    probs = torch.softmax(0.1 * torch.randn(300, 42, generator=g), 1).numpy()
    return probs, Oracle(probs, 20, 41)


def test_long_and_ragged_inputs_make_prefixes_re_enter_the_beam():
    """A prefix that left the beam and comes back must find its old node in the table: the inputs below do that."""
    oracles = [long_case(i)[1] for i in range(3)] + [ragged_case(i)[1] for i in range(len(RAGGED_LENGTHS))]
    print("re-entries", [o.stats["reentries"] for o in oracles], "folds", [o.stats["folds"] for o in oracles],
          "best", [float(o.out[0][0]) for o in oracles])
    print("rejoined", [o.stats["rejoined"] for o in oracles])
    assert sum(o.stats["reentries"] for o in oracles) >= 3
    # ... and some of them meet a child that stayed in the beam: only then does having the old node back change the result
    assert sum(o.stats["rejoined"] for o in oracles) >= 1
    assert sum(o.stats["folds"] for o in oracles) >= 3
    assert all(float(o.out[0][0]) >= 1.1754944e-38 for o in oracles)      # the best score stays a normal f32


def test_8192_frames_in_a_batch_of_three():
    """t_max at its limit: node numbers up to 1 + 8192 * 4, the back-walk over thousands of labels, and the tables and node
    arrays of three sequences side by side in scratch.  Row 1 stops at 8000 frames: padding of a long row."""
    batch = torch.full((3, 8192, 8), NAN)
    for i in range(3):
        batch[i, :LONG_LENGTHS[i]] = torch.from_numpy(long_case(i)[0][:LONG_LENGTHS[i]])
    assert all(not long_case(i)[1].tie and len(long_case(i)[1].out[0][1]) > 500 for i in range(3))
    assert all(long_case(i)[1].stats["nodes"] > len(long_case(i)[1].out[0][1]) > 1000 for i in range(3))
    full = search(batch, LONG_LENGTHS, 4, 7)
    best = search(batch, LONG_LENGTHS, 4, 7, best_only=True)
    assert full[2].shape == (3, 4, 8192) and best[2].shape == (3, 1, 8192)
    for i in range(3):
        equals_oracle(full, i, long_case(i)[1])
        equals_oracle(best, i, long_case(i)[1], best_only=True)


def test_ragged_batch_of_1024_frames_with_nan_behind_the_lengths():
    """[N, 1024, 42] with lengths 1, 2, 127, 128, 129, 1024 and one row of 300 frames whose scores underflow; NaN beyond the
    lengths.  Every row against the oracle on its own frames, all rows and best_only."""
    rows = [ragged_case(i) for i in range(len(RAGGED_LENGTHS))] + [underflow_case()]
    lengths = [p.shape[0] for p, _ in rows]
    assert lengths == list(RAGGED_LENGTHS) + [300]
    under = underflow_case()[1]
    print("underflow: levels", set(map(str, under.stats["levels"])), "last group", under.stats["groups"][-1])
    assert under.tie and float(under.out[0][0]) == 0.0
    last = under.stats["groups"][-1]                  # all candidates at 0: 20 * 42 slots less at most one fold per beam entry
    assert last["frame"] == 299 and 20 * 42 - 20 < last["size"] <= 20 * 42 and last["lo"] == 0
    assert not any(o.tie for _, o in rows[:-1])
    batch = torch.full((len(rows), 1024, 42), NAN)
    for i, (p, _) in enumerate(rows):
        batch[i, :p.shape[0]] = torch.from_numpy(p)
    full = search(batch, lengths, 20, 41)
    best = search(batch, lengths, 20, 41, best_only=True)
    for i, (_, oracle) in enumerate(rows):
        equals_oracle(full, i, oracle)
        equals_oracle(best, i, oracle, best_only=True)
    assert torch.equal(full[4], best[4]) and full[4].tolist() == [0] * len(RAGGED_LENGTHS) + [1]


# --------------------------------------------------------------------------- 5. saturated rows
def test_saturated_rows_with_exact_zeros():
    g = torch.Generator().manual_seed(3)
    probs = torch.softmax(40.0 * torch.randn(30, 42, generator=g), 1).numpy()
    oracle = Oracle(probs, 20, 41)
    zeros = float((probs == 0).mean())
    print("zeros", zeros, "best", float(oracle.out[0][0]), "tie", oracle.tie, "levels", oracle.stats["levels"])
    assert zeros > 0.2 and float(oracle.out[0][0]) > 0
    equals_oracle(search(probs, None, 20, 41), 0, oracle)


# --------------------------------------------------------------------------- 6. blank position and small nKeep
def small_rows(P, blank, seed):
    """Four sequences of 5 frames: two random ones, one that repeats a non-blank symbol with no blank between (distinct
    probabilities per frame, no ties), one that alternates symbol and blank."""
    g = torch.Generator().manual_seed(seed)
    sym = (blank + 1) % P
    rnd = torch.softmax(1.5 * torch.randn(2, 5, P, generator=g), 2)
    rep = torch.softmax(torch.randn(5, P, generator=g) * 0.3, 1) * 0.2
    rep[:, sym] += 0.8
    alt = torch.softmax(torch.randn(5, P, generator=g) * 0.3, 1) * 0.2
    alt[0::2, sym] += 0.8
    alt[1::2, blank] += 0.8
    return torch.cat([rnd, rep[None], alt[None]]).numpy()


def test_every_blank_position_with_the_smallest_beams():
    """nKeep 1, 2, 3; blank first, in the middle, last; P 2 and 3.  Some returned prefix holds a symbol twice in a row: its
    score came through the extension by the prefix's own last symbol, which takes pb alone (no blank between means no repeat)."""
    combos = sorted({(P, blank, k) for P in (2, 3) for blank in (0, P // 2, P - 1) for k in (1, 2, 3)})
    assert len(combos) == 15
    doubled = 0
    for P, blank, n_keep in combos:
        batch = small_rows(P, blank, 100 * P + 10 * blank + n_keep)
        res = search(batch, None, n_keep, blank)
        for n in range(batch.shape[0]):
            oracle = Oracle(batch[n], n_keep, blank)
            doubled += sum(1 for _, lab in oracle.out if any(a == b for a, b in zip(lab, lab[1:])))
            equals_oracle(res, n, oracle)
    assert doubled >= 3


# --------------------------------------------------------------------------- 7. lengths outside [1, T]
def test_lengths_outside_1_to_T_are_clamped():
    """PINNED, as the kernel does it: a length above T decodes T frames; a length of 0 (or below) decodes nothing and returns
    the empty prefix with score 1.0, counts = 1 and no tie."""
    probs = peaked(5, 9, 6, 0.9)
    oracle = Oracle(probs, 4, 5)
    short = Oracle(probs[:3], 4, 5)
    batch = np.stack([probs] * 6)
    lengths = torch.tensor([9, 10, 2 ** 31 - 1, 0, -3, 3], dtype=torch.int64)
    for best_only in (False, True):
        res = search(batch, lengths, 4, 5, best_only=best_only)
        for n in (0, 1, 2):
            equals_oracle(res, n, oracle, best_only)
        equals_oracle(res, 5, short, best_only)
        for n in (3, 4):
            assert rows_of(*res[:4], n) == [(int(np.float32(1.0).view(np.uint32)), [])]
            assert int(res[3][n]) == 1 and int(res[4][n]) == 0 and int(res[1][n, 0]) == 0


# --------------------------------------------------------------------------- alignment score
COSTS = [(-1, -1, 0), (-2, -3, 1)]
STRIP_LENGTHS = (1, 63, 64, 65, 127, 128, 129, 200)


def dev(x, dtype=torch.int32):
    return torch.as_tensor(np.asarray(x), dtype=dtype).to(DEV)


def score(s1, l1, s2, l2, d, m, r):
    out = sa.align_score_batch(dev(s1), dev(l1), dev(s2), dev(l2), d, m, r)
    assert out.dtype == torch.int32 and out.shape == (len(l1),)
    return out.cpu().tolist()


def test_alignment_with_empty_sequences():
    rng = np.random.default_rng(1)
    s1, s2 = rng.integers(0, 5, (4, 70)), rng.integers(0, 5, (4, 90))
    l1, l2 = [0, 70, 0, 33], [90, 0, 0, 65]
    for d, m, r in COSTS + [(3, -1, 2)]:
        assert score(s1, l1, s2, l2, d, m, r) == [-(90 * d), -(70 * d), 0, per_oracle.align_score(s1[3, :33], s2[3, :65], d, m, r)]
        # a matrix without columns: every sequence of that side is empty
        assert score(s1[:, :0], [0, 0, 0, 0], s2, l2, d, m, r) == [-(90 * d), 0, 0, -(65 * d)]
        assert score(s1, l1, s2[:, :0], [0, 5, 0, 0], d, m, r) == [0, -(70 * d), 0, -(33 * d)]
        assert score(s1[:, :0], [0] * 4, s2[:, :0], [0] * 4, d, m, r) == [0] * 4
    per = sa.get_seq_PER_batch(dev(s1), dev(l1), dev(s2), dev(l2)).cpu().numpy()
    assert per.dtype == np.float64 and np.isposinf(per[0]) and per[1] == 1.0 and np.isnan(per[2])
    assert per[3] == per_oracle.get_seq_PER(s1[3, :33], s2[3, :65])


@pytest.mark.parametrize("d,m,r", COSTS)
def test_alignment_at_the_strip_boundaries(d, m, r):
    """Every pair of lengths around 64 and 128 columns (and rows), in one launch."""
    rng = np.random.default_rng(2)
    pairs = [(a, b) for a in STRIP_LENGTHS for b in STRIP_LENGTHS]
    s1, s2 = rng.integers(0, 5, (len(pairs), 200)), rng.integers(0, 5, (len(pairs), 200))
    s2[::3, :150] = s1[::3, :150]                               # a third of the pairs mostly match
    l1, l2 = [a for a, _ in pairs], [b for _, b in pairs]
    want = [per_oracle.align_score(s1[i, :a], s2[i, :b], d, m, r) for i, (a, b) in enumerate(pairs)]
    assert score(s1, l1, s2, l2, d, m, r) == want
    assert sa.align_score_batch(dev(s1, torch.int64), dev(l1, torch.int64), dev(s2, torch.int64), dev(l2, torch.int64), d, m,
                                r).cpu().tolist() == want


def test_alignment_lengths_outside_the_matrix():
    """A length beyond the matrix width counts as the width, a negative one as 0, beside ordinary rows."""
    rng = np.random.default_rng(4)
    s1, s2 = rng.integers(0, 5, (6, 70)), rng.integers(0, 5, (6, 130))
    l1, l2 = [70, 71, 5000, -1, 40, 2 ** 31 - 1], [130, 100, 131, 90, -7, -2 ** 31]
    eff1, eff2 = [70, 70, 70, 0, 40, 70], [130, 100, 130, 90, 0, 0]
    for d, m, r in COSTS:
        want = [per_oracle.align_score(s1[i, :eff1[i]], s2[i, :eff2[i]], d, m, r) for i in range(6)]
        assert want[3] == -(90 * d) and want[4] == -(40 * d)
        assert score(s1, l1, s2, l2, d, m, r) == want
        assert sa.align_score_batch(dev(s1), dev(l1, torch.int64), dev(s2), dev(l2, torch.int64), d, m, r).cpu().tolist() == want


def test_alignment_at_4096_labels():
    """The widest matrices the entry takes, against closed forms (the Python oracle is too slow for 4096 x 4096) and one
    4096 x 64 pair against the oracle."""
    rng = np.random.default_rng(5)
    same = rng.integers(0, 40, (1, 4096))
    for d, m, r in [(-2, -3, 1), (-1, -1, 0), (-1, -1, -1)]:    # r >= d + d: a diagonal of matches is the best path
        assert score(same, [4096], same, [4096], d, m, r) == [-(4096 * r)]
    # disjoint alphabets, unit costs: the edit distance is the longer length
    low, high = rng.integers(0, 20, (3, 4096)), rng.integers(20, 40, (3, 4096))
    assert score(low, [4096, 4096, 70], high, [4096, 70, 4096], -1, -1, 0) == [4096, 4096, 4096]
    assert score(low, [4095, 1, 4096], high, [1, 4095, 0], -1, -1, 0) == [4095, 4095, 4096]
    a, b = rng.integers(0, 5, (1, 4096)), rng.integers(0, 5, (1, 64))
    assert score(a, [4096], b, [64], -2, -3, 1) == [per_oracle.align_score(a[0], b[0], -2, -3, 1)]
    assert score(b, [64], a, [4096], -2, -3, 1) == [per_oracle.align_score(b[0], a[0], -2, -3, 1)]


def test_alignment_refuses_more_than_4096_columns_by_name():
    """PINNED: the entry takes matrices of up to 4096 columns.  The whole-utterance evaluation hands it the search's label rows,
    which are as wide as the utterance batch (up to 8192 frames): beyond 4096 that is this refusal, not a wrong score."""
    wide, narrow = torch.zeros(1, 4097, dtype=torch.int32, device=DEV), torch.zeros(1, 8, dtype=torch.int32, device=DEV)
    one = torch.ones(1, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match=r"align_score: sequences of up to 4096 labels \(ld1=4097 ld2=8\)"):
        sa.align_score_batch(wide, one, narrow, one, -1, -1, 0)
    with pytest.raises(ValueError, match=r"align_score: sequences of up to 4096 labels \(ld1=8 ld2=4097\)"):
        sa.align_score_batch(narrow, one, wide, one, -1, -1, 0)
    found = torch.full((1, 8192), -1, dtype=torch.int32, device=DEV)                # a best_only label row of 8192 frames
    with pytest.raises(ValueError, match=r"align_score: sequences of up to 4096 labels \(ld1=8 ld2=8192\)"):
        sa.get_seq_PER_batch(narrow, one, found, one)
    assert sa.align_score_batch(wide[:, :4096], one, narrow, one, -1, -1, 0).cpu().tolist() == [0]


def test_alignment_at_the_cost_limits():
    """|d|, |m|, |r| = 32768: -(4096 * 32768) in closed form, 300 x 300 against the oracle with every sign, and a positive gap
    cost (the prefix-maximum form of the row update holds for either sign of d)."""
    big = 32768
    rng = np.random.default_rng(6)
    same = rng.integers(0, 40, (1, 4096))
    assert score(same, [4096], same, [4096], -big, -big, big) == [-(4096 * big)]
    assert score(same, [4096], same[:, :0], [0], big, -big, -big) == [-(4096 * big)]
    assert score(same, [4096], same[:, :0], [0], -big, big, big) == [4096 * big]
    s1, s2 = rng.integers(0, 5, (2, 300)), rng.integers(0, 5, (2, 300))
    s2[1, 20:280] = s1[1, 10:270]
    for d, m, r in [(-big, -big, big), (big, big, -big), (-big, big, -big), (big, -big, big), (2, -3, 1), (1, 5, -4)]:
        want = [per_oracle.align_score(s1[i], s2[i, :300 - 37 * i], d, m, r) for i in range(2)]
        assert score(s1, [300, 300], s2, [300, 263], d, m, r) == want, (d, m, r)


def test_alignment_refuses_costs_beyond_32768_by_name():
    s = torch.zeros(1, 8, dtype=torch.int32, device=DEV)
    one = torch.ones(1, dtype=torch.int32, device=DEV)
    for costs, word in [((32769, -1, 0), "d=32769"), ((-32769, -1, 0), "d=-32769"), ((-1, 32769, 0), "m=32769"),
                        ((-1, -32769, 0), "m=-32769"), ((-1, -1, 32769), "r=32769"), ((-1, -1, -32769), "r=-32769")]:
        with pytest.raises(ValueError, match=r"align_score: costs of magnitude up to 32768 \(.*\b%s\b" % word):
            sa.align_score_batch(s, one, s, one, *costs)
