"""The definition of cpc2_amd.spectral (include/cpc2_hip.h) in numpy float64, and per element the bound
the device result is held to.  numpy.fft.rfft on the reflected, windowed frames; nothing here shares code with the package.

The bound, with u = 2^-53, gamma = (n_fft + 2) u, S_t = sum_n |w[n] xr_t[n]|, eps = 2^-24 and the common factor 2 the issue
allows for second-order terms (the f64 matrix instruction's own accumulation is not round-to-nearest):
  linear mel  bM[t,m] = 2 gamma S_t^2 sum_k fb[k,m] + (n_freqs + 2) u M[t,m]
  dB          bD[t,m] = (10 / ln 10) bM / max(M, 10^(floor/10), 1e-10), never below the bound of the element that sets the floor
  mel output  2 bD + eps |v|
  mfcc output 2 (sum_m |dct[k,m]| bD[t,m] + (n_mels + 2) u sum_m |dct[k,m] D[t,m]|) + eps |v|
  deltas      eps |v| (the inputs are the stored f32 values)
"""
import math

import numpy as np

U = 2.0 ** -53
EPS = 2.0 ** -24
SECOND_ORDER = 2.0
AMIN = 1e-10


def window(n_fft):
    return 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)


def twiddles(n_fft):
    """(cos, sin) [n_fft, n_freqs] of 2 pi ((n k) mod n_fft) / n_fft."""
    n = np.arange(n_fft)[:, None]
    k = np.arange(n_fft // 2 + 1)[None, :]
    arg = 2.0 * np.pi * ((n * k) % n_fft).astype(np.float64) / n_fft
    return np.cos(arg), np.sin(arg)


def mel_filterbank(n_fft, n_mels, sample_rate=16000, f_min=0.0, f_max=None):
    """[n_freqs, n_mels], HTK scale, norm=None."""
    f_max = float(sample_rate // 2) if f_max is None else float(f_max)
    n_freqs = n_fft // 2 + 1
    all_freqs = np.linspace(0.0, float(sample_rate // 2), n_freqs)
    # The mel points go through the C library's scalar log10 and pow (math.log10, float ** float), not numpy's vector forms: an
    # entry near a filter's foot is a difference of nearly equal numbers, so one ulp in a point (which two implementations of
    # log10 or pow may well differ by) is thousands of ulps there, and about as much in M as the whole bound bM allows.
    m_pts = np.linspace(2595.0 * math.log10(1.0 + f_min / 700.0), 2595.0 * math.log10(1.0 + f_max / 700.0), n_mels + 2)
    f_pts = np.array([700.0 * (10.0 ** (float(m) / 2595.0) - 1.0) for m in m_pts])
    delta = f_pts[1:] - f_pts[:-1]
    s = f_pts[None, :] - all_freqs[:, None]
    down = -s[:, :-2] / delta[:-1]
    up = s[:, 2:] / delta[1:]
    return np.maximum(0.0, np.minimum(down, up))


def dct_matrix(n_out, n_mels):
    """[n_out, n_mels], type II, norm="ortho"."""
    m = np.arange(n_mels, dtype=np.float64)[None, :]
    k = np.arange(n_out, dtype=np.float64)[:, None]
    d = np.cos(np.pi / n_mels * (m + 0.5) * k) * np.sqrt(2.0 / n_mels)
    d[0] *= 1.0 / np.sqrt(2.0)
    return d


def grid_of(name, hop):
    """(offset, frames(L)) of a named frame grid."""
    if name == "cpc":
        return hop // 2, lambda L: L // hop
    if name == "center":
        return 0, lambda L: 1 + L // hop
    raise ValueError(name)


def frame_indices(L, n_fft, hop, offset, T):
    """[T, n_fft] sample indices after reflection (no edge sample repeated)."""
    if L <= n_fft // 2:
        raise ValueError("reflection needs L > n_fft // 2")
    i = (np.arange(T)[:, None] * hop + offset - n_fft // 2) + np.arange(n_fft)[None, :]
    i = np.where(i < 0, -i, i)
    i = np.where(i >= L, 2 * (L - 1) - i, i)
    assert T == 0 or (i.min() >= 0 and i.max() < L)
    return i


def linear_mel(x, n_fft, hop, offset, T, fb):
    """(M [T, n_mels], bM) of one signal."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 1
    frames = x.astype(np.float64)[frame_indices(len(x), n_fft, hop, offset, T)] * window(n_fft)[None, :]
    P = np.abs(np.fft.rfft(frames, n=n_fft, axis=1)) ** 2
    M = P @ fb
    S = np.abs(frames).sum(axis=1)
    bM = 2.0 * (n_fft + 2) * U * (S ** 2)[:, None] * fb.sum(axis=0)[None, :] + (fb.shape[0] + 2) * U * M
    return M, bM


def features(signals, kind="mfcc", n_fft=400, hop=160, n_mels=40, n_out=13, grid="cpc", sample_rate=16000, f_min=0.0,
             f_max=None, top_db=80.0, floor="signal"):
    """Per signal (value [T, n_out or n_mels] float64, bound): the mel (dB) or mfcc output and what the device is held to."""
    offset, frames_of = grid_of(grid, hop)
    fb = mel_filterbank(n_fft, n_mels, sample_rate, f_min, f_max)
    lin = [linear_mel(x, n_fft, hop, offset, frames_of(len(x)), fb) for x in signals]
    dbs = [10.0 * np.log10(np.maximum(M, AMIN)) for M, _ in lin]
    out = []
    if top_db is None:
        floors = [(-np.inf, 0.0)] * len(lin)
    else:
        def top(group):
            """(floor, bound of the element that sets it) over the signals of `group`."""
            best, b_best = -np.inf, 0.0
            for i in group:
                M, bM = lin[i]
                if M.size and dbs[i].max() > best:
                    j = np.unravel_index(np.argmax(dbs[i]), M.shape)
                    best, b_best = dbs[i][j], 10.0 / np.log(10.0) * bM[j] / max(M[j], AMIN)
            return best - top_db, b_best
        if floor == "call":
            floors = [top(range(len(lin)))] * len(lin)
        elif floor == "signal":
            floors = [top([i]) for i in range(len(lin))]
        else:
            raise ValueError(floor)
    dct = dct_matrix(n_out, n_mels) if kind == "mfcc" else None
    for (M, bM), D, (fl, b_fl) in zip(lin, dbs, floors):
        D = np.maximum(D, fl)
        bD = 10.0 / np.log(10.0) * bM / np.maximum(np.maximum(M, 10.0 ** (fl / 10.0)), AMIN)
        bD = np.maximum(bD, b_fl)
        if kind == "mel":
            out.append((D, SECOND_ORDER * bD + EPS * np.abs(D)))
        else:
            C = D @ dct.T
            b = bD @ np.abs(dct).T + (n_mels + 2) * U * (np.abs(D) @ np.abs(dct).T)
            out.append((C, SECOND_ORDER * b + EPS * np.abs(C)))
    return out


def deltas(c):
    """One order of deltas of stored f32 rows [T, D] in float64 (replicate edges); the device is held to eps |v|."""
    c = np.asarray(c)
    assert c.dtype == np.float32 and c.ndim == 2
    c = c.astype(np.float64)
    T = c.shape[0]
    at = lambda s: c[np.clip(np.arange(T) + s, 0, T - 1)]       # noqa: E731
    return ((at(1) - at(-1)) + 2.0 * (at(2) - at(-2))) / 10.0
