"""The ABX kernels on the MI355X at the sizes an evaluation uses, against the fp64 oracle (tests/abx_oracle.py) and numpy:
work lists of more than 8192 segments (every workgroup of cpc_abx_dtw, cpc_abx_dtw_units and cpc_abx_counts takes a second
and a third segment and reuses its scratch), triplets of the command line's group sizes (8000 and 27 000 comparisons),
three and four strips of ordinary frames, scratch that holds NaN before the launch, and the refusals of the dense entry
points.

Path length and value are compared with the oracle on CLEAR pairs: those whose fp64 backtrack never chose between two
predecessors closer than 1e-5 relative (abx_oracle.dtw_margin), the scale of the f32 error of a running cost.  Every test
that uses this also caps the share of unclear pairs, so it cannot pass by comparing nothing.  Inputs whose costs are exact
integers, and unit ids, have no unclear pair: every pair is compared, ties included."""
import numpy as np
import pytest
import torch

from cpc2_amd import _lib
from cpc2_amd.eval.ABX import abx_group_computation as abx_g
from cpc2_amd.eval.ABX import abx_iterators as abx_it
from tests import abx_oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
COS, EUC = abx_g.get_cosine_distance_batch, abx_g.get_euclidian_distance_batch
CAP = 8192                                                    # workgroups per launch of the three kernels
CLEAR = 1e-5


# --------------------------------------------------------------------------- inputs and oracle tables
def _normalised(rng, n, D):
    """n normalised frames of D columns (D - 1 drawn, plus the singularity column)."""
    v = torch.from_numpy(rng.standard_normal((n, D - 1)).astype(np.float32))
    return abx_it.normalize_with_singularity(v).numpy()


def _integer_frames(rng, n, D=8, column=5):
    """Frames whose only non-zero coordinate holds an integer in -3..3, all in the same column: the euclidian distance of
    two frames is |a - b|, an exact integer, and so is every running cost, in f32 as in fp64."""
    v = np.zeros((n, D), dtype=np.float32)
    v[:, column] = rng.integers(-3, 4, n)
    return v


def _frames(kind, rng, n):
    if kind == "exact":
        return _integer_frames(rng, n)
    if kind == "cosine":
        return _normalised(rng, n, 36)                       # dp = 36: a whole 32-wide chunk and a partial one
    return rng.standard_normal((n, 33)).astype(np.float32)   # dp = 36 again, three columns of padding


def _distance(kind):
    return "cosine" if kind == "cosine" else "euclidian"


def _runs(rng, n, n_units):
    out = []
    while len(out) < n:
        out += [int(rng.integers(0, n_units))] * int(rng.integers(1, 6))
    return np.array(out[:n], dtype=np.int64)


def _oracle_table(xs, ys, dist_rows):
    """dtw_margin of every (x, y): value, path length and margin as [len(xs), len(ys)] arrays.  dist_rows(x) is the fp64
    frame-distance matrix of x against all frames of ys, concatenated."""
    off = np.concatenate([[0], np.cumsum([len(y) for y in ys])])
    V = np.empty((len(xs), len(ys)))
    L = np.empty((len(xs), len(ys)), dtype=np.int64)
    M = np.empty((len(xs), len(ys)))
    for i, x in enumerate(xs):
        d = dist_rows(x)
        for j in range(len(ys)):
            V[i, j], L[i, j], M[i, j] = O.dtw_margin(d[:, off[j]:off[j + 1]])
    return V, L, M


def _dense_table(xs, ys, distance):
    all_y = np.concatenate(ys)
    return _oracle_table(xs, ys, lambda x: O.frame_distances(x, all_y, distance))


def _unit_table(xs, ys, d_same, d_diff):
    all_y = np.concatenate(ys)
    same, diff = np.float64(np.float32(d_same)), np.float64(np.float32(d_diff))
    return _oracle_table(xs, ys, lambda x: np.where(np.asarray(x)[:, None] == all_y[None, :], same, diff))


def _assert_exact(vals, plen, v, n):
    """Every pair: the oracle's path length, and its value to the one f32 division the kernel rounds in."""
    bad = np.flatnonzero(plen != n)
    assert bad.size == 0, (bad[:5], plen[bad[:5]], n[bad[:5]])
    bad = np.flatnonzero(~(np.abs(vals - v) <= 2e-7 * np.abs(v)))
    assert bad.size == 0, (bad[:5], vals[bad[:5]], v[bad[:5]])


def _assert_clear(vals, plen, v, n, margin):
    """Clear pairs: test_dtw_kernel_matches_oracle's bound on the value, and the oracle's path length."""
    clear = margin >= CLEAR
    bad = np.flatnonzero(clear & ~(np.abs(vals - v) < 1e-5 * np.maximum(1.0, np.abs(v))))
    assert bad.size == 0, (bad[:5], vals[bad[:5]], v[bad[:5]])
    bad = np.flatnonzero(clear & (plen != n))
    assert bad.size == 0, (bad[:5], plen[bad[:5]], n[bad[:5]], margin[bad[:5]])


# --------------------------------------------------------------------------- A. work lists past the grid cap
POOL_LENS = [1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 7, 8, 9, 10, 12, 15, 20, 25, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 14, 16, 17, 18,
             19, 21, 22, 23, 65, 70, 130]
N_POOL = len(POOL_LENS)
P65, P70, P130 = 37, 38, 39                                   # the pool's items of more than one strip
N_SEG = 2 * CAP + 37
# (x pool item, y pool items) of segments s, s + 8192 and s + 16384: what ONE workgroup runs one after the other
PLACED = {
    3: ((P130, [P65, 3]), (P65, [P130]), (P70, [P65, 20, P130])),              # long, long, long; ly differs every time
    5: ((P70, [P130, 0]), (6, [P130, 2]), (P130, [36, P70])),                  # long, short, long
    7: ((0, [5]), (P130, [P70, 1, P65]), (2, [1])),                            # short, long, short
    # y lists of more than 8, 4 and 4: every wave of the unit kernel takes a second pair after a multi-strip one
    11: ((P130, [P65, P70, 10, 0, 36, 25, 1, 30, 35]), (P65, [0, P130, 1, P70, 2, 36]), (P70, [P65, P130, 36, 35, 34])),
    13: ((10, [3]), (P65, [P70]), (P130, [1, P70, 0])),                        # short, long; one-frame y around a long one
    36: ((P130, [P65]), (P130, [4]), (P130, [P70])),                           # the last workgroup that takes a third segment
}


@pytest.fixture(scope="module")
def work():
    """(x pool item of every segment [N_SEG], px, py): item i < N_POOL is pool item i, item N_POOL + s is the x of segment
    s, an alias of pool item xp[s] (same frames, an item of its own, so that it is a segment of its own).  No x meets the
    pool item it aliases: under the cosine distance an item against itself sits where acos is singular, and the f32 dot
    product moves a frame distance by up to 2e-4 there (test_dtw_kernel_near_identical_frames of test_abx_gpu.py holds that
    case to its own bound); the bounds here are those of independent frames."""
    rng = np.random.default_rng(20)
    xp = rng.integers(0, P65, N_SEG)                           # short x; the long ones are placed
    ys = [rng.choice(N_POOL - 1, int(k), replace=False) for k in rng.integers(1, 4, N_SEG)]
    ys = [(y + (y >= x)).tolist() for x, y in zip(xp, ys)]     # 1 to 3 distinct pool items other than xp[s]
    for s, laps in PLACED.items():
        for lap, (x, y) in enumerate(laps):
            xp[s + lap * CAP] = x
            ys[s + lap * CAP] = y
    px = np.concatenate([np.full(len(y), N_POOL + s, dtype=np.int64) for s, y in enumerate(ys)])
    py = np.concatenate([np.asarray(y, dtype=np.int64) for y in ys])
    assert len(np.unique(px)) == N_SEG > 2 * CAP and (np.diff(px) >= 0).all() and (xp[px - N_POOL] != py).all()
    return xp, px, py


def _alias_offsets(xp):
    pool_off = np.concatenate([[0], np.cumsum(POOL_LENS)[:-1]])
    lens = np.concatenate([POOL_LENS, np.asarray(POOL_LENS)[xp]])
    off = np.concatenate([pool_off, pool_off[xp]])
    return (torch.from_numpy(off.astype(np.int32)).to(DEV), torch.from_numpy(lens.astype(np.int32)).to(DEV), lens)


def _dense_items(pool, xp):
    rows = np.concatenate(pool)
    dp = -(-rows.shape[1] // 4) * 4
    frames = torch.zeros(rows.shape[0], dp, dtype=torch.float32, device=DEV)
    frames[:, :rows.shape[1]] = torch.from_numpy(rows)
    off, lens, lens_host = _alias_offsets(xp)
    return abx_g._Items(frames, off, lens, lens_host)


def _unit_items(pool, xp, distances):
    units = torch.from_numpy(np.concatenate(pool).astype(np.int32)).to(DEV)
    off, lens, lens_host = _alias_offsets(xp)
    return abx_g._UnitItems(units, off, lens, lens_host, distances)


def _dense_pool(kind, seed):
    rng = np.random.default_rng(seed)
    return [_frames(kind, rng, n) for n in POOL_LENS]


def _expected(table, xp, px, py):
    return tuple(t[xp[px - N_POOL], py] for t in table)


def _unclear_share(M, xp, px, py):
    """Share of unclear pairs among the distinct (pool x, pool y) of the work list."""
    used = np.zeros(M.shape, dtype=bool)
    used[xp[px - N_POOL], py] = True
    return ((M < CLEAR) & used).sum() / used.sum()


WORK_SEED = 0


@pytest.mark.parametrize("kind", ["exact", "cosine", "euclidian"])
def test_dense_kernel_past_the_grid_cap(work, kind):
    """16 421 segments on 8192 workgroups: every workgroup reuses its boundary rows for a second segment, 37 for a third.
    exact: every pair is held to the oracle's path length and to 2e-7 on the value (integer costs; ties resolve alike).
    cosine (D = 36) and euclidian (D = 33), dp = 36: clear pairs only, and at most 2 % of the distinct pairs unclear.  The
    oracle alone, default_rng(0), on the 1467 distinct pairs of the work list: 8 unclear for cosine and 8 for euclidian
    (0.55 % each)."""
    xp, px, py = work
    pool = _dense_pool(kind, WORK_SEED)
    items = _dense_items(pool, xp)
    assert items.frames.size(1) == (8 if kind == "exact" else 36)
    vals, plen = abx_g._dtw_pairs(items, px, py, abx_g.COSINE if kind == "cosine" else abx_g.EUCLIDIAN)
    vals, plen = vals.cpu().numpy().astype(np.float64), plen.cpu().numpy()
    table = _dense_table(pool, pool, _distance(kind))
    v, n, margin = _expected(table, xp, px, py)
    if kind == "exact":
        assert np.abs(table[0] * table[1] - np.round(table[0] * table[1])).max() < 1e-9  # integer costs indeed
        _assert_exact(vals, plen, v, n)
    else:
        share = _unclear_share(table[2], xp, px, py)
        print(f"{kind}: {share:.4%} of the distinct pairs unclear")
        assert share <= 0.02
        _assert_clear(vals, plen, v, n, margin)


def test_unit_kernel_past_the_grid_cap(work):
    """The same work list on unit ids (n_units = 8, cosine: frame distances 0 and 0.5, every cost exact): one wave per
    pair, so the boundary rows of a WAVE are reused across segments, and with the y lists of 5 to 9 across the pairs of
    one segment.  Value and path length equal the oracle's for every pair."""
    xp, px, py = work
    rng = np.random.default_rng(WORK_SEED)
    pool = [_runs(rng, n, 8) for n in POOL_LENS]
    d_same, d_diff = abx_g.unit_frame_distances(8, True, COS)
    assert (d_same, d_diff) == (0.0, 0.5)
    items = _unit_items(pool, xp, {abx_g.COSINE: (d_same, d_diff)})
    vals, plen = abx_g._dtw_pairs(items, px, py, abx_g.COSINE)
    vals, plen = vals.cpu().numpy(), plen.cpu().numpy()
    v, n, _ = _expected(_unit_table(pool, pool, d_same, d_diff), xp, px, py)
    bad = np.flatnonzero((vals != v.astype(np.float32)) | (plen != n))
    assert bad.size == 0, (bad[:5], vals[bad[:5]], v[bad[:5]], plen[bad[:5]], n[bad[:5]])


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def test_dense_kernel_reads_no_scratch_it_has_not_written(work):
    """The entry point itself on the same work list, its scratch of exactly cpc_abx_dtw_scratch_bytes filled with 0xFF
    bytes (NaN as a cost, -1 as a length): bit for bit what _dtw_pairs gives on the arena's scratch."""
    xp, px, py = work
    items = _dense_items(_dense_pool("cosine", WORK_SEED), xp)
    vals, plen = abx_g._dtw_pairs(items, px, py, abx_g.COSINE)
    seg_x, seg_start, d_py, n_seg, max_lx, max_ly = abx_g._segment_lists(items, px, py)
    assert (n_seg, max_lx, max_ly) == (N_SEG, 130, 130)
    lib = _lib.load()
    nbytes = lib.cpc_abx_dtw_scratch_bytes(n_seg, max_lx, max_ly)
    assert nbytes == CAP * 2 * 130 * 8
    scratch = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    out = torch.full((len(px),), 7.0, dtype=torch.float32, device=DEV)
    out_len = torch.full((len(px),), 7, dtype=torch.int32, device=DEV)
    _lib.check(lib.cpc_abx_dtw(_lib.ptr(items.frames), items.frames.size(1), _lib.ptr(items.off), _lib.ptr(items.lens),
                               items.n, _lib.ptr(seg_x), _lib.ptr(seg_start), _lib.ptr(d_py), n_seg, max_lx, max_ly,
                               abx_g.COSINE, _lib.ptr(out), _lib.ptr(out_len), _lib.ptr(scratch), nbytes,
                               _lib.stream_ptr(DEV)), "cpc_abx_dtw")
    assert not torch.isnan(out).any()
    assert torch.equal(_bits(out), _bits(vals)) and torch.equal(out_len, plen)


def test_unit_kernel_reads_no_scratch_it_has_not_written(work):
    """cpc_abx_dtw_units on the same work list with 0xFF scratch of exactly cpc_abx_dtw_units_scratch_bytes."""
    xp, px, py = work
    rng = np.random.default_rng(WORK_SEED)
    d_same, d_diff = 0.0, 0.5
    items = _unit_items([_runs(rng, n, 8) for n in POOL_LENS], xp, {abx_g.COSINE: (d_same, d_diff)})
    vals, plen = abx_g._dtw_pairs(items, px, py, abx_g.COSINE)
    seg_x, seg_start, d_py, n_seg, max_lx, max_ly = abx_g._segment_lists(items, px, py)
    lib = _lib.load()
    nbytes = lib.cpc_abx_dtw_units_scratch_bytes(n_seg, max_lx, max_ly)
    assert nbytes == CAP * 4 * 2 * 130 * 8
    scratch = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    out = torch.full((len(px),), 7.0, dtype=torch.float32, device=DEV)
    out_len = torch.full((len(px),), 7, dtype=torch.int32, device=DEV)
    _lib.check(lib.cpc_abx_dtw_units(_lib.ptr(items.units), _lib.ptr(items.off), _lib.ptr(items.lens), items.n,
                                     _lib.ptr(seg_x), _lib.ptr(seg_start), _lib.ptr(d_py), n_seg, max_lx, max_ly, d_same,
                                     d_diff, _lib.ptr(out), _lib.ptr(out_len), _lib.ptr(scratch), nbytes,
                                     _lib.stream_ptr(DEV)), "cpc_abx_dtw_units")
    assert not torch.isnan(out).any()
    assert torch.equal(_bits(out), _bits(vals)) and torch.equal(out_len, plen)


# --------------------------------------------------------------------------- B. cpc_abx_counts against numpy
N_TRIP = 2 * CAP + 5
BIG_SHAPES = [(1, 1, 1), (7, 9, 11), (5, 20, 30), (20, 20, 20), (30, 30, 30)]       # nx, na, nb


def test_counts_kernel_against_numpy():
    """16 389 triplets on 8192 workgroups, most of 1 to 27 comparisons; workgroups 0 to 4 take three of the shapes
    (1,1,1) (7,9,11) (5,20,30) (20,20,20) (30,30,30) one after the other, small before large and large before small: up
    to 106 trips of the 256-wide entry loop, after and before a triplet that takes one.  (20,20,20) and (30,30,30) carry the
    symmetric case's -1 diagonal; some indices point past the pair results.  dist is full of ties and holds NaN.  lt and
    eq equal numpy's counts for every triplet."""
    rng = np.random.default_rng(3)
    n_pairs = 5000
    dist = rng.choice(np.array([0.125, 0.25, 0.5, 0.75], dtype=np.float32), n_pairs)
    cont = rng.random(n_pairs) < 0.25
    dist[cont] = rng.random(int(cont.sum()), dtype=np.float32)
    dist[rng.random(n_pairs) < 0.03] = np.nan
    shapes = [tuple(int(v) for v in s) for s in rng.integers(1, 4, (N_TRIP, 3))]
    for t in range(5):
        for lap in range(3):
            shapes[t + lap * CAP] = BIG_SHAPES[(t + 2 * lap) % 5]
    ia_l, ib_l, shape = [], [], np.zeros((N_TRIP, 5), dtype=np.int32)
    a_off = b_off = 0
    for t, (nx, na, nb) in enumerate(shapes):
        ia = rng.integers(0, n_pairs, (nx, na)).astype(np.int32)
        ib = rng.integers(0, n_pairs, (nx, nb)).astype(np.int32)
        if nx == na and na >= 20:
            ia[np.arange(na), np.arange(na)] = -1              # the symmetric case's excluded diagonal
        if t % 97 == 0 or nx * na * nb > 1000:                 # indices past the pair results: skipped, not read
            ia[rng.integers(0, nx), rng.integers(0, na)] = n_pairs + int(rng.integers(0, 3)) * 1000
            ib[rng.integers(0, nx), rng.integers(0, nb)] = (n_pairs, 2 ** 31 - 1)[t % 2]
        shape[t] = (nx, na, nb, a_off, b_off)
        ia_l.append(ia)
        ib_l.append(ib)
        a_off += ia.size
        b_off += ib.size
    lt = torch.full((N_TRIP,), -7, dtype=torch.int32, device=DEV)
    eq = torch.full((N_TRIP,), -7, dtype=torch.int32, device=DEV)
    d_dist = torch.from_numpy(dist).to(DEV)
    d_ia = torch.from_numpy(np.concatenate([v.reshape(-1) for v in ia_l])).to(DEV)
    d_ib = torch.from_numpy(np.concatenate([v.reshape(-1) for v in ib_l])).to(DEV)
    d_shape = torch.from_numpy(shape).to(DEV)
    _lib.check(_lib.load().cpc_abx_counts(_lib.ptr(d_dist), n_pairs, _lib.ptr(d_ia), _lib.ptr(d_ib), _lib.ptr(d_shape),
                                          N_TRIP, _lib.ptr(lt), _lib.ptr(eq), _lib.stream_ptr(DEV)), "cpc_abx_counts")
    lt, eq = lt.cpu().numpy(), eq.cpu().numpy()
    want_lt, want_eq = np.empty(N_TRIP, dtype=np.int64), np.empty(N_TRIP, dtype=np.int64)
    for t, (ia, ib) in enumerate(zip(ia_l, ib_l)):
        ok_a, ok_b = (ia >= 0) & (ia < n_pairs), (ib >= 0) & (ib < n_pairs)
        a = dist[np.where(ok_a, ia, 0)][:, :, None]
        b = dist[np.where(ok_b, ib, 0)][:, None, :]
        ok = ok_a[:, :, None] & ok_b[:, None, :]
        want_lt[t] = ((a < b) & ok).sum()                      # NaN compares false
        want_eq[t] = ((a == b) & ok).sum()
    assert want_eq.max() > 1000 and want_lt.max() > 5000      # the ties and the sizes are there
    bad = np.flatnonzero((lt != want_lt) | (eq != want_eq))
    assert bad.size == 0, (bad[:5], lt[bad[:5]], want_lt[bad[:5]], eq[bad[:5]], want_eq[bad[:5]])


# --------------------------------------------------------------------------- C. full groups through the package
def _padded(items):
    S = max(v.shape[0] for v in items)
    out = torch.zeros(len(items), S, items[0].shape[1])
    for i, v in enumerate(items):
        out[i, :v.shape[0]] = torch.from_numpy(np.asarray(v, dtype=np.float32))
    return out.to(DEV), torch.tensor([v.shape[0] for v in items])


def _group(rng, n):
    return [_normalised(rng, int(k), 9) for k in rng.integers(3, 26, n)]      # D = 8 drawn, normalised


@pytest.mark.parametrize("mode", ["within", "across"])
def test_theta_of_full_size_groups_within_oracle_band(mode):
    """get_theta_group_dtw on groups of the command line's default size: 20 x 19 x 20 comparisons within (x = a, the
    diagonal excluded), 5 x 20 x 20 across.  theta within the oracle's band for comparisons closer than 1e-4 (+- 1e-6,
    as test_batched_scores_within_oracle_band_and_reference_scores); the band is narrower than 0.01.  The oracle alone,
    default_rng(5): 0.0017 wide within, 0.0035 across."""
    rng = np.random.default_rng(5)
    symmetric = mode == "within"
    a, b = _group(rng, 20), _group(rng, 20)
    x = a if symmetric else _group(rng, 5)
    (ta, sa), (tb, sb), (tx, sx) = _padded(a), _padded(b), _padded(x)
    theta = abx_g.get_theta_group_dtw(ta, tb, tx, sa, sb, sx, COS, symmetric)
    want, dxa, dxb = O.triplet_theta(a, b, x, "cosine", symmetric)
    n_norm = (20 * 19 if symmetric else 20 * 5) * 20
    lo, hi = O.theta_band(dxa, dxb, n_norm, 1e-4)
    print(f"{mode}: theta {theta} oracle {want} band [{lo}, {hi}]")
    assert lo <= want <= hi and hi - lo < 0.01
    assert lo - 1e-6 <= theta <= hi + 1e-6


@pytest.mark.parametrize("symmetric", [False, True])
def test_score_triplets_does_not_depend_on_the_chunking(symmetric):
    """30 full-size triplets over one item store: one chunk (the default max_pairs) and one chunk per triplet
    (max_pairs = 1) give the same thetas bit for bit."""
    rng = np.random.default_rng(6)
    store = _group(rng, 70)
    items = abx_g._Items.from_padded([_padded(store)], DEV)
    trips = []
    for _ in range(30):
        pick = rng.permutation(70).tolist()
        a, b = pick[:20], pick[20:40]
        trips.append((a, b, a if symmetric else pick[40:45]))
    one, many = {}, {}
    whole = abx_g._score_triplets(items, trips, symmetric, abx_g.COSINE, stats=one)
    split = abx_g._score_triplets(items, trips, symmetric, abx_g.COSINE, max_pairs=1, stats=many)
    assert (one["chunks"], many["chunks"]) == (1, 30)
    assert whole.dtype == torch.float32 and torch.equal(whole.view(torch.int32), split.view(torch.int32))
    assert 0.0 < float(whole.min()) and float(whole.max()) < 1.0 and len(set(whole.tolist())) > 20


# --------------------------------------------------------------------------- D. three and four strips of ordinary frames
STRIP_X = [128, 129, 192, 193]                                 # two strips exactly, one row of a third, three, a fourth
STRIP_Y = [1, 64, 65, 128, 129, 200]
STRIP_SEED = 11


def _strip_pairs(kind, rng):
    """The 24 pairs in one work list through cpc_abx_dtw, and the oracle's table."""
    xs = [_frames(kind, rng, n) for n in STRIP_X]
    ys = [_frames(kind, rng, n) for n in STRIP_Y]
    items = abx_g._Items.from_padded([_padded(xs), _padded(ys)], DEV)
    assert items.frames.size(1) == (8 if kind == "exact" else 36)
    px = np.repeat(np.arange(len(xs)), len(ys))
    py = np.tile(np.arange(len(ys)), len(xs)) + len(xs)
    vals, plen = abx_g._dtw_pairs(items, px, py, abx_g.COSINE if kind == "cosine" else abx_g.EUCLIDIAN)
    table = _dense_table(xs, ys, _distance(kind))
    return vals.cpu().numpy().astype(np.float64), plen.cpu().numpy(), tuple(t.reshape(-1) for t in table)


def test_dense_kernel_strips_exact():
    """Integer costs over 2, 3 and 4 strips and 1 to 4 column tiles: every pair has the oracle's path length, and its
    value to 2e-7."""
    vals, plen, (v, n, _) = _strip_pairs("exact", np.random.default_rng(STRIP_SEED))
    assert np.abs(v * n - np.round(v * n)).max() < 1e-9             # integer costs indeed
    _assert_exact(vals, plen, v, n)


def test_dense_kernel_strips_continuous():
    """Ordinary frames, cosine (D = 36) and euclidian (D = 33), dp = 36: clear pairs have the oracle's value and path
    length; at most 25 % of the 48 pairs are unclear (paths of up to 392 cells accumulate costs near 1000, where 1e-5
    relative is 0.01).  The oracle alone, default_rng(11): 4 of 48 unclear (3 cosine, 1 euclidian), 8.3 %."""
    rng = np.random.default_rng(STRIP_SEED)
    unclear = 0
    for kind in ("cosine", "euclidian"):
        vals, plen, (v, n, margin) = _strip_pairs(kind, rng)
        unclear += int((margin < CLEAR).sum())
        _assert_clear(vals, plen, v, n, margin)
    print(f"{unclear} of 48 pairs unclear")
    assert unclear <= 0.25 * 48


# --------------------------------------------------------------------------- E. refusals of the dense entry points
def _edge_call(lib, items, scratch, nbytes):
    # segments x = 0 (5 frames), 1 (70 frames), 9 (no such item); pairs:
    #   (0, 2) (0, 4: no such item) (0, -1) (0, 3) | (1, 2) (1, 3: 80 frames > max_len_y) (1, 1) (1, 0) | (9, 0)
    seg_x = torch.tensor([0, 1, 9], dtype=torch.int32, device=DEV)
    seg_start = torch.tensor([0, 4, 8, 9], dtype=torch.int32, device=DEV)
    pair_y = torch.tensor([2, 4, -1, 3, 2, 3, 1, 0, 0], dtype=torch.int32, device=DEV)
    vals = torch.zeros(9, dtype=torch.float32, device=DEV)
    plen = torch.zeros(9, dtype=torch.int32, device=DEV)
    _lib.check(lib.cpc_abx_dtw(_lib.ptr(items.frames), items.frames.size(1), _lib.ptr(items.off), _lib.ptr(items.lens),
                               items.n, _lib.ptr(seg_x), _lib.ptr(seg_start), _lib.ptr(pair_y), 3, 70, 70, abx_g.EUCLIDIAN,
                               _lib.ptr(vals), _lib.ptr(plen), _lib.ptr(scratch), nbytes, _lib.stream_ptr(DEV)),
               "cpc_abx_dtw")
    return vals.cpu().numpy(), plen.cpu().numpy()


def test_dense_entry_points_uncomputable_pairs_and_bad_arguments():
    rng = np.random.default_rng(5)
    frames = [_integer_frames(rng, n) for n in (5, 70, 9, 80)]
    items = abx_g._Items.from_padded([_padded(frames)], DEV)
    lib = _lib.load()
    nbytes = lib.cpc_abx_dtw_scratch_bytes(3, 70, 70)
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)

    def check_edges():
        vals, plen = _edge_call(lib, items, scratch, nbytes)
        nan, ok = [1, 2, 5, 8], [0, 3, 4, 6, 7]
        assert np.isnan(vals[nan]).all() and (plen[nan] == -1).all()
        want = [O.dtw_items(frames[x], frames[y], "euclidian") for x, y in ((0, 2), (0, 3), (1, 2), (1, 1), (1, 0))]
        _assert_exact(vals[ok].astype(np.float64), plen[ok], np.array([w[0] for w in want]), np.array([w[1] for w in want]))
        assert vals[6] == 0.0 and plen[6] == 70                # an item against itself: the diagonal

    check_edges()
    one = torch.zeros(16, dtype=torch.int32, device=DEV)
    rows = torch.zeros(16, dtype=torch.float32, device=DEV)
    outv = torch.zeros(4, dtype=torch.float32, device=DEV)

    def call(frames=rows, dp=4, n_items=1, max_lx=4, max_ly=4, distance=abx_g.COSINE, out=outv):
        return lib.cpc_abx_dtw(_lib.ptr(frames), dp, _lib.ptr(one), _lib.ptr(one), n_items, _lib.ptr(one), _lib.ptr(one),
                               _lib.ptr(one), 1, max_lx, max_ly, distance, _lib.ptr(out), None, None, 0,
                               _lib.stream_ptr(DEV))
    for kwargs, word in (({"dp": 6}, "multiple of 4"), ({"dp": 0}, "multiple of 4"), ({"distance": 2}, "unknown distance"),
                         ({"frames": None}, "null buffer"), ({"out": None}, "null buffer"), ({"n_items": 0}, "bad sizes"),
                         ({"max_ly": 0}, "bad sizes"), ({"max_lx": 65}, "scratch")):
        with pytest.raises(ValueError, match=word):
            _lib.check(call(**kwargs), "cpc_abx_dtw")
    check_edges()                                              # a refusal leaves the next valid call intact

    assert lib.cpc_abx_dtw_scratch_bytes(10, 64, 500) == 0
    assert lib.cpc_abx_dtw_scratch_bytes(10, 65, 500) >= 10 * 2 * 500 * 8
    assert lib.cpc_abx_dtw_scratch_bytes(20000, 65, 500) == lib.cpc_abx_dtw_scratch_bytes(CAP, 65, 500) == CAP * 2 * 500 * 8

    lt = torch.full((4,), 77, dtype=torch.int32, device=DEV)
    eq = torch.full((4,), 77, dtype=torch.int32, device=DEV)

    def counts(dist=rows, n_pairs=16, n_trip=1, lt=lt):
        return lib.cpc_abx_counts(_lib.ptr(dist), n_pairs, _lib.ptr(one), _lib.ptr(one), _lib.ptr(one), n_trip, _lib.ptr(lt),
                                  _lib.ptr(eq), _lib.stream_ptr(DEV))
    for kwargs, word in (({"dist": None}, "null buffer"), ({"lt": None}, "null buffer"), ({"n_pairs": 0}, "bad sizes")):
        with pytest.raises(ValueError, match=word):
            _lib.check(counts(**kwargs), "cpc_abx_counts")
    _lib.check(counts(n_trip=0), "cpc_abx_counts")             # nothing to do: OK, and nothing written
    torch.cuda.synchronize()
    assert (lt == 77).all() and (eq == 77).all()
    _lib.check(counts(), "cpc_abx_counts")                     # a triplet of shape (0, 0, 0): no comparison
    torch.cuda.synchronize()
    assert lt.tolist() == [0, 77, 77, 77] and eq.tolist() == [0, 77, 77, 77]
