"""cpc_moments_accumulate (csrc/moments.hip) on the GPU: the streaming f64 second moments against numpy -- exactly on integer
data, within the first-order bound of an f64 sum on data with a large offset, and through the cancellation of a centred
covariance, which a float32 accumulation misses by about 1e-1."""
import numpy as np
import pytest
import torch

import cca_oracle as CO
from cpc2_amd import _lib
from cpc2_amd._lib import check, ptr, scratch, stream_ptr
from cpc2_amd.cca import Moments

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

SHAPES = [(1, 1, 0), (3, 5, 0), (5, 12, 10), (63, 16, 16), (64, 17, 15), (257, 3, 1), (4099, 64, 48), (1031, 256, 256),
          (257, 512, 512), (130, 512, 0)]


def _accumulate(x, ldx, dx, y, ldy, dy, n, sums, gram):
    lib = _lib.load()
    nb = lib.cpc_moments_scratch_bytes(n, dx, dy)
    assert nb > 0
    check(lib.cpc_moments_accumulate(ptr(x), ldx, dx, ptr(y), ldy, dy, n, ptr(sums), ptr(gram), ptr(scratch(nb, DEV)), nb,
                                     stream_ptr(DEV)), "moments_accumulate")


def _fresh(d):
    return torch.zeros(d, dtype=torch.float64, device=DEV), torch.zeros(d, d, dtype=torch.float64, device=DEV)


def _run(x, y):
    """One call on contiguous host arrays x [n, dx], y [n, dy] or None -> (sums, gram) as numpy."""
    n, dx = x.shape
    dy = 0 if y is None else y.shape[1]
    xd = torch.from_numpy(x).to(DEV)
    yd = None if y is None else torch.from_numpy(y).to(DEV)
    sums, gram = _fresh(dx + dy)
    _accumulate(xd, dx, dx, yd, dy, dy, n, sums, gram)
    return sums.cpu().numpy(), gram.cpu().numpy()


def _offset_data(n, dx, dy, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, dx)) + 1000.0).astype(np.float32)
    y = (rng.standard_normal((n, dy)) + 1000.0).astype(np.float32) if dy else None
    return x, y


def _stack(x, y):
    return x if y is None else np.concatenate([x, y], axis=1)


@pytest.mark.parametrize("n,dx,dy", SHAPES)
def test_integer_inputs_give_the_exact_moments(n, dx, dy):
    """Integers in [-64, 64]: every product and every partial sum is an exact f64 integer, so the result must EQUAL numpy's
    int64 Z^T Z and column sums whatever the order of summation -- a wrong lane map or a dropped row cannot hide."""
    rng = np.random.default_rng(1000 * n + dx)
    zi = rng.integers(-64, 65, size=(n, dx + dy), dtype=np.int64)
    x = zi[:, :dx].astype(np.float32)
    y = zi[:, dx:].astype(np.float32) if dy else None
    sums, gram = _run(np.ascontiguousarray(x), None if y is None else np.ascontiguousarray(y))
    assert np.array_equal(sums, zi.sum(0).astype(np.float64))
    assert np.array_equal(gram, (zi.T @ zi).astype(np.float64))
    assert np.array_equal(gram, gram.T)


@pytest.mark.parametrize("n,dx,dy", [(257, 3, 1), (4099, 64, 48), (1031, 256, 256), (130, 512, 0)])
def test_offset_inputs_within_the_f64_sum_bound(n, dx, dy):
    """randn + 1000:  |gram - oracle| <= 2 n 2^-53 (|Z|^T |Z|) elementwise, and the same form for the sums."""
    x, y = _offset_data(n, dx, dy, seed=n + dx)
    sums, gram = _run(x, y)
    _, sx, sy, Sxx, Sxy, Syy = CO.moments(x, y)
    ref_s = np.concatenate([sx, sy])
    ref_g = np.block([[Sxx, Sxy], [Sxy.T, Syy]])
    bs, bg = CO.moments_bound(x, y)
    print("gram error / bound", (np.abs(gram - ref_g) / bg).max(), "sums error / bound", (np.abs(sums - ref_s) / bs).max())
    assert (np.abs(gram - ref_g) <= bg).all()
    assert (np.abs(sums - ref_s) <= bs).all()
    assert np.array_equal(gram, gram.T)


def test_centred_covariance_survives_the_cancellation():
    """n = 4099 rows of randn + 1000: the raw moments are about 4e9 and the covariance about 1, so forming it cancels nine
    digits.  From the f64 moments it is within 1e-9 of the covariance of the centred data (relative to its largest entry); a
    float32 accumulation of the same products is off by about 1e-1.  Measured: 4.6e-10 (2.4e-9 with one chain of the f64 matrix
    instruction per 256 rows, whose accumulation truncates: DESIGN.md section 17)."""
    n, dx, dy = 4099, 64, 48
    x, y = _offset_data(n, dx, dy, seed=n + dx)
    sums, gram = _run(x, y)
    z = _stack(x, y).astype(np.float64)
    zc = z - z.mean(0)
    ref = zc.T @ zc / (n - 1)
    cov = (gram - np.outer(sums, sums) / n) / (n - 1)
    err = np.abs(cov - ref).max() / np.abs(ref).max()
    print("centred covariance: relative error", err)
    # (for the record: the signed error of the raw moments against exact integer arithmetic -- every input is a multiple of 2^-14)
    zi = np.round(z * 2.0 ** 14).astype(np.int64)
    signed = ((gram * 2.0 ** 28).astype(np.int64) - zi.T @ zi) / 2.0 ** 28
    print("raw moments: signed error mean %.3e, min %.3e, max %.3e" % (signed.mean(), signed.min(), signed.max()))
    assert err <= 1e-9


def test_running_totals_and_reproducible_bits():
    n, dx, dy = 4099, 64, 48
    x, y = _offset_data(n, dx, dy, seed=5)
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    _, one = _run(x, y)
    h = n // 2

    def halves():
        sums, gram = _fresh(dx + dy)
        _accumulate(xd, dx, dx, yd, dy, dy, h, sums, gram)
        _accumulate(xd[h:], dx, dx, yd[h:], dy, dy, n - h, sums, gram)
        return sums.cpu().numpy(), gram.cpu().numpy()

    s1, g1 = halves()
    s2, g2 = halves()
    assert np.array_equal(g1, g2) and np.array_equal(s1, s2)            # the same calls, the same bits
    bs, bg = CO.moments_bound(x, y)
    assert (np.abs(g1 - one) <= bg).all()
    _, sx, sy, Sxx, Sxy, Syy = CO.moments(x, y)
    assert (np.abs(g1 - np.block([[Sxx, Sxy], [Sxy.T, Syy]])) <= bg).all()
    assert (np.abs(s1 - np.concatenate([sx, sy])) <= bs).all()
    assert np.array_equal(g1, g1.T)


def test_row_strides_are_passed_on_not_copied():
    n, dx, dy = 257, 17, 15
    rng = np.random.default_rng(11)
    xb = rng.integers(-64, 65, size=(n, dx + 3)).astype(np.float32)
    yb = rng.integers(-64, 65, size=(n, dy + 5)).astype(np.float32)
    xd, yd = torch.from_numpy(xb).to(DEV), torch.from_numpy(yb).to(DEV)
    sums, gram = _fresh(dx + dy)
    _accumulate(xd, dx + 3, dx, yd, dy + 5, dy, n, sums, gram)
    zi = np.concatenate([xb[:, :dx], yb[:, :dy]], axis=1).astype(np.int64)
    assert np.array_equal(gram.cpu().numpy(), (zi.T @ zi).astype(np.float64))
    assert np.array_equal(sums.cpu().numpy(), zi.sum(0).astype(np.float64))
    # the same through Moments, as a [b, s, d] view of wider rows and as a 2-D slice
    m = Moments(dx, dy, device=DEV)
    b, s = 3, 40
    m.update(xd[:b * s].view(b, s, dx + 3)[:, :, :dx], yd[:b * s].view(b, s, dy + 5)[:, :, :dy])
    m.update(xd[b * s:, :dx], yd[b * s:, :dy])
    assert m.count == n
    count, sx, sy, Sxx, Sxy, Syy = m.state()
    assert np.array_equal(np.block([[Sxx, Sxy], [Sxy.T, Syy]]), (zi.T @ zi).astype(np.float64))
    assert np.array_equal(np.concatenate([sx, sy]), zi.sum(0).astype(np.float64))


def test_y_may_alias_x():
    n, d = 1031, 70
    x, _ = _offset_data(n, d, 0, seed=2)
    xd = torch.from_numpy(x).to(DEV)
    sums, gram = _fresh(2 * d)
    _accumulate(xd, d, d, xd, d, d, n, sums, gram)
    g = gram.cpu().numpy()
    assert np.array_equal(g[:d, d:], g[:d, :d]) and np.array_equal(g[d:, d:], g[:d, :d])
    s = sums.cpu().numpy()
    assert np.array_equal(s[:d], s[d:])
    _, bg = CO.moments_bound(x)
    assert (np.abs(g[:d, :d] - CO.moments(x)[3]) <= bg).all()


def test_moments_refuses_host_tensors():
    m = Moments(4, 3, device=DEV)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.update(torch.zeros(5, 4), torch.zeros(5, 3))
