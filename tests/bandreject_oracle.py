"""The numpy statement of the `bandreject_sinc` filter (cpc2_amd.data_augmentation.BandrejectSincAugment's docstring and
include/cpc2_hip.h state the same thing): a Kaiser-windowed sinc band-reject FIR of 2 H + 1 taps, symmetric about the output
sample, and the band draw of the reference's BandrejectAugment.generate_freq_mask.  It is written from that definition alone,
imports nothing of the package, and everything in it is float64 (np.i0, np.sinc, np.convolve).

  beta = 0.1102 (A - 8.7)   dw = 2 pi tbw / sr   M = ceil((A - 7.95) / (2.285 dw))   H = (M + 1) // 2   T = 2 H + 1
  w[j] = I0(beta sqrt(1 - (j / H)^2)) / I0(beta)   lp_f[j] = (2 f / sr) sinc(2 f j / sr)   h[j] = [j == 0] - w[j] (lp_high[j] - lp_low[j])
  y[t] = sum_{j = -H .. H} h[j] x[t - j], x zero outside [0, W)"""
import math

import numpy as np

SR = 16000.0


def design(attenuation_dB=120.0, transition_hz=400.0, sr=SR):
    """(beta, M, H, T) of an attenuation in dB and a transition width in Hz."""
    beta = 0.1102 * (attenuation_dB - 8.7)
    dw = 2 * math.pi * transition_hz / sr
    order = int(math.ceil((attenuation_dB - 7.95) / (2.285 * dw)))
    half = (order + 1) // 2
    return beta, order, half, 2 * half + 1


def is_band(low, high, sr=SR):
    return bool(0 <= low <= high <= sr / 2)                    # (False for a NaN)


def taps(low, high, half, beta, sr=SR):
    """h[-H .. H] (2 H + 1 values, float64) of the band (low, high).  An empty band, or a pair that is no band, gives the identity."""
    j = np.arange(-half, half + 1, dtype=np.float64)
    delta = (j == 0).astype(np.float64)
    if not is_band(low, high, sr) or low == high:
        return delta
    w = np.i0(beta * np.sqrt(1 - (j / half) ** 2)) / np.i0(beta)
    lp = lambda f: (2 * f / sr) * np.sinc(2 * f * j / sr)                                # noqa: E731
    return delta - w * (lp(high) - lp(low))


def bandreject(x, low, high, half, beta, sr=SR):
    """y [B, W] (float64, NOT rounded) of the windows x [B, W] (float32 values) with the bands (low[i], high[i])."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    assert x.ndim == 2
    low = np.broadcast_to(np.asarray(low, dtype=np.float64), (x.shape[0],))
    high = np.broadcast_to(np.asarray(high, dtype=np.float64), (x.shape[0],))
    y = np.empty_like(x)
    for i in range(x.shape[0]):
        if not is_band(low[i], high[i], sr) or low[i] == high[i]:
            y[i] = x[i]
        else:
            y[i] = np.convolve(x[i], taps(low[i], high[i], half, beta, sr))[half:half + x.shape[1]]
    return y


def reach(x, half):
    """sum_j |x[t - j]| over the filter's support, [B, W] in float64: what a sample's rounding errors scale with."""
    a = np.abs(np.asarray(x, dtype=np.float32).astype(np.float64))
    c = np.concatenate([np.zeros((a.shape[0], 1)), np.cumsum(a, axis=1)], axis=1)
    t = np.arange(a.shape[1])
    return c[:, np.minimum(t + half + 1, a.shape[1])] - c[:, np.maximum(t - half, 0)]


def response(h, freqs, sr=SR):
    """|H(f)| of symmetric taps h[-H .. H] at the frequencies `freqs` (Hz)."""
    half = (len(h) - 1) // 2
    j = np.arange(1, half + 1, dtype=np.float64)
    f = np.asarray(freqs, dtype=np.float64)
    return np.abs(h[half] + 2 * np.cos(2 * np.pi * f[:, None] * j[None, :] / sr) @ h[half + 1:])


def mel2freq(mel):
    return (10 ** (mel / 2595) - 1) * 700


def draw(scaler=1.0):
    """(low, high) of one window: two np.random.uniform calls on the mel scale."""
    width = 27 * scaler
    melfmax = 2595 * np.log10(1 + 8000 / 700)
    meldf = np.random.uniform(0, melfmax * width / 256)
    melf0 = np.random.uniform(0, melfmax - meldf)
    return float(mel2freq(melf0)), float(mel2freq(melf0 + meldf))


def apply_plan(plan, lo, hi, clean):
    """Rows [lo, hi) of a sealed bandreject_sinc plan applied to the windows `clean` [hi - lo, W]: float64, not rounded."""
    assert plan["kind"] == "bandreject_sinc"
    return bandreject(clean, plan["low"][lo:hi], plan["high"][lo:hi], plan["half"], plan["beta"])
