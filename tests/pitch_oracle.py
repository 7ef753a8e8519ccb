"""The float64 statement of the `pitch_wsola` pitch shift (cpc2_amd.data_augmentation.PitchShiftAugment's docstring and
include/cpc2_hip.h state it in words), in vectorised numpy, with the first-order error bound the f32 device path is held to.

A window x[0 .. W) reads as zero outside [0, W).  r = 2 ** (cents / 1200); cents == 0 returns the window.  Stage 1 is a WSOLA
stretch by r given as a function s(m) of segment starts q_j; stage 2 resamples it by r through a Hann-windowed sinc.

The search is exact, not approximate: a candidate's cost is the last element of np.cumsum over k of (x[cand + k] - t[k]) ** 2 in
float64 -- one addition per term with k ascending, the kernel's order -- so the device's q must EQUAL this one's, near-ties
included, and np.argmin's first minimum is the lowest candidate.

The bound.  u = 2 ** -24.  The device rounds every weight once to f32, takes a cross-faded sample in f64 and rounds it once, and
adds the products in one f32 fmaf chain; this statement keeps all of that in f64.  Per output, with the sums over its taps:
    bound = sum |h| E_s + (taps + 2) u sum |h| |s| + DELTA_TRIG sum |s|
E_s = 3 u (|a| + |b|) inside an overlap (the cross-fade a + (k / O) (b - a)) and 0 elsewhere (a raw sample is exact); `taps`
rounding errors of the chain plus one for the weight's rounding and one to spare; DELTA_TRIG = 2 ** -40 is the allowance for the
absolute error of a weight as the device's f64 sin / cos (and its tap-to-tap rotation of them) give it.  DELTA_TRIG is ASSUMED:
no documented accuracy of the device's f64 sin / cos is at hand; OpenCL's full profile allows 4 ulp, which with 26 rotations of
4 roundings each stays below 1e-13, and 2 ** -40 = 9.1e-13 is ten times that and still 1e-5 of the f32 terms beside it."""
import numpy as np

S, O, R = 1312, 192, 234
HO = S - O
L, ROLLOFF = 6, 0.99
TAP_GUARD = 16
U = 2.0 ** -24
DELTA_TRIG = 2.0 ** -40


def ratio_of(cents):
    return 2.0 ** (int(cents) / 1200.0)


def cutoff_of(r):
    return ROLLOFF * min(1.0, 1.0 / r)


def segments(window, cents):
    """J: segments of HO stretched samples that cover every tap of every output (the largest tap lies below
    (W - 1) r + L / c < ceil(W r) + 16 for |cents| <= 1200)."""
    reach = int(np.ceil(window * ratio_of(cents))) + TAP_GUARD
    return -(-reach // HO)


def nominal_starts(cents, count):
    """p_j = floor(j HO / r + 0.5), j < count (p_0 is never used: q_0 = 0)."""
    return np.floor(np.arange(count, dtype=np.float64) * HO / ratio_of(cents) + 0.5).astype(np.int64)


def tables(cents, window, count=None):
    """What PitchShiftAugment.seal / data_augmentation.pitch_tables build for a batch: cents, ratio, cutoff, nominal [n, J]."""
    cents = [int(c) for c in cents]
    J = max([segments(window, c) for c in cents] + [1, int(count or 1)])
    ratio = np.array([ratio_of(c) for c in cents], dtype=np.float64)
    return {"cents": np.array(cents, dtype=np.int32), "ratio": ratio,
            "cutoff": np.array([cutoff_of(r) for r in ratio], dtype=np.float64),
            "nominal": np.stack([nominal_starts(c, J) for c in cents]).astype(np.int32) if cents else np.zeros((0, J), np.int32)}


def _read(x, i):
    """x[i] with zeros outside [0, len(x))."""
    i = np.asarray(i)
    ok = (i >= 0) & (i < len(x))
    return np.where(ok, x[np.clip(i, 0, len(x) - 1)], 0.0)


def search(x, cents, count=None):
    """The chain q_0 .. q_{J-1} of a window (float32 values, held in float64)."""
    xd = np.asarray(x, dtype=np.float32).astype(np.float64)
    J = max(segments(len(xd), cents), int(count or 1))
    p = nominal_starts(cents, J)
    q = np.zeros(J, dtype=np.int64)
    for j in range(1, J):
        first = p[j] - R // 2
        t = _read(xd, q[j - 1] + HO + np.arange(O))
        span = _read(xd, first + np.arange(R + O - 1))
        cand = np.lib.stride_tricks.sliding_window_view(span, O)              # [R, O]: candidate d is span[d : d + O]
        cost = np.cumsum((cand - t[None, :]) ** 2, axis=1)[:, -1]
        q[j] = first + int(np.argmin(cost))
    return q


def stretched(x, q, m):
    """s(m) for m >= 0, and E_s / u of the bound: 3 (|a| + |b|) inside an overlap, 0 elsewhere."""
    xd = np.asarray(x, dtype=np.float32).astype(np.float64)
    j = m // HO
    k = m - j * HO
    jc = np.minimum(j, len(q) - 1)                           # (a live tap never lies beyond the table; dead ones are masked by the caller)
    b = _read(xd, q[jc] + k)
    a = _read(xd, q[np.maximum(jc - 1, 0)] + HO + k)
    fade = (k < O) & (j >= 1)
    s = np.where(fade, a + (k / O) * (b - a), b)
    return s, np.where(fade, 3.0 * (np.abs(a) + np.abs(b)), 0.0)


def pitch(x, cents, count=None):
    """(y [W] float64, q [J] int64, bound [W] float64) of one window."""
    xd = np.asarray(x, dtype=np.float32).astype(np.float64)
    W = len(xd)
    q = search(xd, cents, count)
    if cents == 0:
        return xd.copy(), q, np.zeros(W)
    r = ratio_of(cents)
    c = cutoff_of(r)
    half = L / c
    pos = np.arange(W, dtype=np.float64) * r
    m0 = np.ceil(pos - half).astype(np.int64)
    y, sum_hs, sum_hes, sum_s, taps = np.zeros(W), np.zeros(W), np.zeros(W), np.zeros(W), np.zeros(W)
    for i in range(int(np.ceil(2 * half)) + 2):
        m = m0 + i
        t = (pos - m) * c
        live = (np.abs(t) < L) & (m >= 0)
        h = np.where(live, c * np.sinc(t) * np.cos(np.pi * t / (2 * L)) ** 2, 0.0)
        s, es = stretched(xd, q, np.maximum(m, 0))
        s, es = np.where(live, s, 0.0), np.where(live, es, 0.0)
        y += h * s
        sum_hs += np.abs(h) * np.abs(s)
        sum_hes += np.abs(h) * es
        sum_s += np.abs(s)
        taps += live
    bound = U * sum_hes + (taps + 2) * U * sum_hs + DELTA_TRIG * sum_s
    return y, q, bound


def pitch_batch(x, cents, count=None):
    """Rows of a [b, W] batch with one shared J (the largest of the batch, as the device tables have it)."""
    x = np.asarray(x)
    cents = [int(c) for c in cents]
    J = max([segments(x.shape[1], c) for c in cents] + [1, int(count or 1)])
    ys, qs, bs = zip(*[pitch(row, c, J) for row, c in zip(x, cents)])
    return np.stack(ys), np.stack(qs), np.stack(bs)


def replay(plan, clean, lo=0, hi=None):
    """Rows [lo, hi) of a sealed pitch_wsola plan applied to the windows `clean` [hi - lo, W]: (y, q, bound)."""
    assert plan["kind"] == "pitch_wsola"
    hi = plan["n"] if hi is None else hi
    return pitch_batch(clean, plan["cents"][lo:hi], plan["nominal"].shape[1])
