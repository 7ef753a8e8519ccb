"""The statements of term detection and term discovery on quantized units (include/cpc2_hip.h): the
definitions of cpc_sdtw and cpc_local_align with d[i][j] replaced by the two-valued distance.  Helper module of
tests/test_term_units_*.py (not a test file).

The distance matrix is built here and handed to tests.sdtw_oracle.sdtw_f32 and tests.lalign_oracle.local_align_f32, which perform
the definition's f32 operations in order.  The distances are given, not computed, so a kernel is held to EQUALITY with them on
every case, ties included: the score as a bit pattern and every span integer.  With two-valued distances nearly every decision
is a tie, so the tie rules are what is being tested."""
import functools
import math

import numpy as np

from tests.lalign_oracle import local_align_f32
from tests.sdtw_oracle import sdtw_f32

SQRT2 = float(np.sqrt(np.float32(2)))
# (d_same, d_diff) with (theta, gamma) of the alignment: the two distances of unit_frame_distances and a pair with d_same > 0
CONFIGS = (((0.0, 0.5), (0.25, 0.125)), ((0.0, SQRT2), (0.25, 0.0)), ((0.125, 0.75), (0.3, 0.1)))
ROW_LENGTHS = (1, 2, 63, 64, 65, 128, 129, 200)       # one to four strips
COL_LENGTHS = (1, 5, 10, 63, 64, 65, 130, 257)        # across the strip seams and the 64-unit refills of the column register
ALPHABETS = (2, 8, 50)
DISJOINT = 1000                                       # added to the units of a column item that shares none with any row item


def distance_matrix(x, y, d_same, d_diff):
    x, y = np.asarray(x), np.asarray(y)
    return np.where(x[:, None] == y[None, :], np.float32(d_same), np.float32(d_diff))


def sdtw_units(x, y, d_same, d_diff):
    """(score f32, start, end, length) of query x inside document y."""
    return sdtw_f32(distance_matrix(x, y, d_same, d_diff))


def local_align_units(x, y, d_same, d_diff, theta, gamma):
    """(score f32, (start_i, end_i, start_j, end_j, length)) of row item x against column item y."""
    return local_align_f32(distance_matrix(x, y, d_same, d_diff), theta, gamma)


def draw_units(rng, n, n_units):
    """n frames of unit ids in runs of 1 .. 5 frames."""
    out = []
    while len(out) < n:
        out += [int(rng.integers(0, n_units))] * int(rng.integers(1, 6))
    return np.asarray(out[:n], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def family():
    """The items of the equality tests: per alphabet one row item per ROW_LENGTHS and one column item per COL_LENGTHS, and one
    more column item over a disjoint alphabet.  Returns (items, pairs): items a list of int32 arrays, pairs a list of (row item,
    column item) indices: every row length against every column length in every alphabet (64 rows against 10 columns and m < n
    among them), and every row item of the first alphabet against the disjoint column item."""
    rng = np.random.default_rng(2929)
    items, pairs = [], []
    for n_units in ALPHABETS:
        rows = [len(items) + k for k in range(len(ROW_LENGTHS))]
        items += [draw_units(rng, n, n_units) for n in ROW_LENGTHS]
        cols = [len(items) + k for k in range(len(COL_LENGTHS))]
        items += [draw_units(rng, m, n_units) for m in COL_LENGTHS]
        pairs += [(a, b) for a in rows for b in cols]
    items.append(draw_units(rng, 70, 8) + DISJOINT)
    pairs += [(a, len(items) - 1) for a in range(len(ROW_LENGTHS))]
    return items, pairs


@functools.lru_cache(maxsize=None)
def family_sdtw(config):
    (d_same, d_diff), _ = CONFIGS[config]
    items, pairs = family()
    return [sdtw_units(items[a], items[b], d_same, d_diff) for a, b in pairs]


@functools.lru_cache(maxsize=None)
def family_align(config):
    (d_same, d_diff), (theta, gamma) = CONFIGS[config]
    items, pairs = family()
    return [local_align_units(items[a], items[b], d_same, d_diff, theta, gamma) for a, b in pairs]


def same_bits(score, want):
    """Whether the f32 `score` has the bit pattern of the statement's np.float32 (NaN included)."""
    return np.float32(score).tobytes() == np.float32(want).tobytes()


def scratch_bytes(n_seg, max_len_row, max_len_col):
    """The boundary rows of the unit entry points: nothing when one strip holds every row item; else per wave of the launch (at most
    2048 workgroups of 4) two rows of max_len_col cells of three words."""
    return 0 if max_len_row <= 64 else min(n_seg, 2048) * 4 * 2 * 12 * max_len_col


assert math.isclose(SQRT2, math.sqrt(2), rel_tol=1e-7)
