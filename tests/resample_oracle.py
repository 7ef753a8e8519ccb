"""fp64 statement of the sample-rate conversion (torchaudio's sinc_interp_hann resampler, which the reference's
cpc/eval/utils/adjust_sample_rate.py applies): what csrc/resample.hip and cpc2_amd.audio.resample are held against.  numpy only.

    g = gcd(orig, new), o = orig / g, n = new / g, base = min(o, n) * rolloff, w = ceil(width * o / base), taps = 2 w + o
    h[p][j] = sinc(t) * cos(t pi / width / 2)^2 * base / o,  t = clamp((-p / n + (j - w) / o) * base, -width, +width)
    y[f n + p] = sum_j h[p][j] * xp[f o + j],  xp = w zeros, x, w + o zeros;  cut to ceil(n L / o) samples"""
import math

import numpy as np


def plan(orig_freq, new_freq, width=6, rolloff=0.99):
    g = math.gcd(int(orig_freq), int(new_freq))
    o, n = int(orig_freq) // g, int(new_freq) // g
    base = min(o, n) * rolloff
    w = int(math.ceil(width * o / base))
    return o, n, w, 2 * w + o


def table(orig_freq, new_freq, width=6, rolloff=0.99):
    """h [n, taps] in float64."""
    o, n, w, taps = plan(orig_freq, new_freq, width, rolloff)
    base = min(o, n) * rolloff
    p = np.arange(n, dtype=np.float64)[:, None]
    j = np.arange(taps, dtype=np.float64)[None, :]
    t = (-p / float(n) + (j - float(w)) / float(o)) * base
    t = np.clip(t, -float(width), float(width))
    win = np.cos(t * math.pi / float(width) / 2.0) ** 2
    safe = np.where(t == 0.0, 1.0, t)
    sinc = np.where(t == 0.0, 1.0, np.sin(math.pi * safe) / (math.pi * safe))
    return sinc * win * base / float(o)


def output_length(length, o, n):
    return -((-n * int(length)) // o)


def padded(x, o, w):
    x = np.asarray(x, dtype=np.float64)
    return np.concatenate([np.zeros(w), x, np.zeros(w + o)])


def _frames(xp, o, taps, frames):
    idx = np.arange(frames)[:, None] * o + np.arange(taps)[None, :]
    return xp[idx]                                                     # [frames, taps]


def resample(x, orig_freq, new_freq, width=6, rolloff=0.99, h=None, with_bound_sum=False):
    """y in float64 (h: a table to apply instead of the float64 one, e.g. the f32-rounded table).  with_bound_sum: also
    sum_j |h[p][j]| |xp[f o + j]| per output sample, the scale of a dot product's rounding error."""
    o, n, w, taps = plan(orig_freq, new_freq, width, rolloff)
    h = table(orig_freq, new_freq, width, rolloff) if h is None else np.asarray(h, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    out_len = output_length(x.shape[-1], o, n)
    frames = -(-out_len // n) if out_len else 0
    xp = padded(x, o, w)
    xp = np.concatenate([xp, np.zeros(max(0, (frames - 1) * o + taps - xp.size))])
    seg = _frames(xp, o, taps, frames)
    y = (seg @ h.T).reshape(-1)[:out_len]
    if not with_bound_sum:
        return y
    return y, (np.abs(seg) @ np.abs(h).T).reshape(-1)[:out_len]
