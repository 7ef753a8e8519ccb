"""The numpy statement of the `freeverb` reverberation (cpc2_amd.data_augmentation.FreeverbAugment's docstring and
include/cpc2_hip.h state the same thing): eight parallel feedback combs with a one-pole low-pass in the loop, four all-passes in
series, sample by sample.  It is written from that definition alone and imports nothing of the package.  One function evaluates it
in float64 or, operation for operation, in float32; the loop over samples is Python's and every operation in it is vectorised over
the windows and the eight combs, so a few windows of 20480 samples take about a second.

  COMB, ALLPASS in samples at 44.1 kHz, rho = 16000 / 44100; per window rs in [0, 100): scale = rs / 100 * 0.9 + 0.1,
  D[c] = int(scale rho COMB[c] + 0.5), A[a] = int(rho ALLPASS[a] + 0.5); fb, dmp, g from (reverberance, hf_damping, wet_gain_dB),
  each rounded once to float32 -- the float64 evaluation uses those rounded values too, so the two differ by arithmetic alone."""
import math

import numpy as np

COMB = (1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617)
ALLPASS = (225, 341, 441, 556)
RHO = 16000 / 44100


def comb_lengths(rs):
    scale = rs / 100 * 0.9 + 0.1
    return tuple(int(scale * RHO * c + 0.5) for c in COMB)


def allpass_lengths():
    return tuple(int(RHO * a + 0.5) for a in ALLPASS)


def scalars(reverberance=100.0, hf_damping=100.0, wet_gain_dB=0.0):
    """(fb, dmp, g) in float64, before their one rounding to float32."""
    a = -1 / math.log(0.7)
    b = 100 / (math.log(0.02) * a + 1)
    fb = 1 - math.exp((reverberance - b) / (a * b))
    dmp = hf_damping / 100 * 0.3 + 0.2
    g = 0.015 * 10 ** (wet_gain_dB / 20)
    return fb, dmp, g


def freeverb(x, rooms, reverberance=100.0, hf_damping=100.0, wet_gain_dB=0.0, dtype=np.float64, comb_len=None):
    """y [B, W] of the windows x [B, W] (float32 values) with room sizes `rooms` [B] (or the comb lengths `comb_len` [B, 8] given
    outright), every operation in `dtype`."""
    x = np.asarray(x, dtype=np.float32)
    assert x.ndim == 2
    B, W = x.shape
    if comb_len is None:
        comb_len = [comb_lengths(int(r)) for r in np.asarray(rooms).reshape(-1)]
    D = np.asarray(comb_len, dtype=np.int64).reshape(B, 8)
    A = allpass_lengths()
    fb, dmp, g = (dtype(np.float32(v)) for v in scalars(reverberance, hf_damping, wet_gain_dB))
    half = dtype(0.5)
    xs = x.astype(dtype)
    u_all = g * xs
    lines = np.zeros((B, 8, int(D.max()) if B else 1), dtype=dtype)
    s = np.zeros((B, 8), dtype=dtype)
    p = np.zeros((B, 8), dtype=np.int64)
    ap_lines = [np.zeros((B, n), dtype=dtype) for n in A]
    pa = [0, 0, 0, 0]
    bi = np.arange(B)[:, None]
    ci = np.arange(8)[None, :]
    y = np.empty((B, W), dtype=dtype)
    for n in range(W):
        u = u_all[:, n]
        o = lines[bi, ci, p]
        s = o + (s - o) * dmp
        lines[bi, ci, p] = u[:, None] + s * fb
        p = (p + 1) % D
        acc = np.zeros(B, dtype=dtype)
        for c in range(8):
            acc = acc + o[:, c]
        v = acc
        for k in range(4):
            line = ap_lines[k]
            o_a = line[:, pa[k]].copy()
            line[:, pa[k]] = v + o_a * half
            v = o_a - v
            pa[k] = (pa[k] + 1) % A[k]
        y[:, n] = xs[:, n] + v
    assert y.dtype == dtype
    return y


def apply_plan(plan, lo, hi, clean, reverberance=100.0, hf_damping=100.0, wet_gain_dB=0.0, dtype=np.float64):
    """Rows [lo, hi) of a sealed freeverb plan applied to the windows `clean` [hi - lo, W], from the rooms it drew."""
    assert plan["kind"] == "freeverb"
    return freeverb(clean, plan["room"][lo:hi], reverberance, hf_damping, wet_gain_dB, dtype)
