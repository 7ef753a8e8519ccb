"""fp64 restatements of the augmentation transforms (cpc/data_augmentation.py :157-228, :268-275, :278-318;
cpc/dataset.py:433-438) and of the replay of a plan (cpc2_amd/data_augmentation.py): what the kernels of csrc/augment.hip and
the loader's augmented batches are held against.  numpy / scipy only; windows are rows of [n, W] float64 arrays."""
import numpy as np
from scipy.signal import fftconvolve

EPS = 1e-8


def peak_norm(w):
    w = np.asarray(w, dtype=np.float64)
    return w / (np.abs(w).max(axis=-1, keepdims=True) + EPS)


def energy_norm(w):
    w = np.asarray(w, dtype=np.float64)
    return w / (np.sqrt(np.mean(w ** 2, axis=-1, keepdims=True)) + EPS)


def gain_of(snr):
    """data_augmentation.py:218-220."""
    return 1.0 / (10.0 ** (np.asarray(snr, dtype=np.float64) / 20.0))


def additive(x, noise, gain, noise_peak_norm=False):
    """peak(e(x) + g e(noise)), row by row; noise_peak_norm: the noise data set's PeakNorm first."""
    noise = np.asarray(noise, dtype=np.float64)
    if noise_peak_norm:
        noise = peak_norm(noise)
    g = np.asarray(gain, dtype=np.float64).reshape(-1, 1)
    return peak_norm(energy_norm(x) + energy_norm(noise) * g)


def natural_reverb(x, responses):
    """Row i: y[t] = sum_{k <= t} ir_i[k] x[t - k], t < W, then peak normalisation; responses[i] None or empty: no convolution."""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty_like(x)
    for i, ir in enumerate(responses):
        if ir is None or len(ir) == 0:
            out[i] = x[i]
        else:
            ir = np.asarray(ir, dtype=np.float64)
            out[i] = fftconvolve(x[i], ir)[:x.shape[1]] if len(ir) > 64 else np.convolve(x[i], ir)[:x.shape[1]]
    return peak_norm(out)


def time_dropout(x, start, length):
    out = np.array(x, dtype=np.float64, copy=True)
    for i, (s, n) in enumerate(zip(start, length)):
        out[i, int(s):int(s) + int(n)] = 0.0
    return out


def _host(t):
    return t.detach().cpu().double().numpy() if hasattr(t, "detach") else np.asarray(t, dtype=np.float64)


def replay(plan, x, lo=0, hi=None, ir_data=None, meta_ir_data=None):
    """Rows [lo, hi) of `plan` applied to the windows x [hi - lo, W] (float64).  ir_data: the flat impulse-response vector of
    the NaturalReverb the plan (or a part of it) came from; meta_ir_data: that of the noise data set's augmentation."""
    hi = plan["n"] if hi is None else hi
    x = np.asarray(x, dtype=np.float64)
    w = x.shape[1]
    kind = plan["kind"]
    if kind == "combined":
        for part in plan["parts"]:
            x = replay(part, x, lo, hi, ir_data, meta_ir_data)
        return x
    if kind == "time_dropout":
        return time_dropout(x, plan["start"][lo:hi], plan["length"][lo:hi])
    if kind == "natural_reverb":
        flat = _host(ir_data)
        responses = [flat[o:o + min(n, w)] if n > 0 else None for o, n in zip(plan["ir_off"][lo:hi], plan["ir_len"][lo:hi])]
        return natural_reverb(x, responses)
    if kind == "additive":
        vectors = [_host(t) for t in plan["noise_data"]]
        noise = np.stack([vectors[s][o:o + w] for s, o in zip(plan["noise_src"][lo:hi], plan["noise_off"][lo:hi])])
        if plan["noise_peak_norm"]:
            noise = peak_norm(noise)
        if plan["meta"] is not None:
            noise = replay(plan["meta"], noise, lo, hi, meta_ir_data, None)
        return additive(x, noise, gain_of(plan["snr"][lo:hi]))
    raise ValueError(kind)


# ----------------------------------------------------------------------------- fixtures the tests write into tmp_path
def write_wav(path, samples, rate=16000):
    """16-bit PCM mono .wav."""
    import os
    import wave
    os.makedirs(os.path.dirname(str(path)), exist_ok=True)
    with wave.open(str(path), "wb") as fh:
        fh.setnchannels(1)
        fh.setsampwidth(2)
        fh.setframerate(rate)
        fh.writeframes((np.clip(np.asarray(samples, dtype=np.float64), -1, 1) * 32767).astype("<i2").tobytes())


def make_noise_db(root, lengths=(30000, 41000, 25000), seed=0, rate=16000):
    """A directory of noise .wav files (coloured noise of different levels); returns the directory."""
    rng = np.random.RandomState(seed)
    for i, n in enumerate(lengths):
        white = rng.randn(n + 8)
        noise = np.convolve(white, np.ones(8) / 8.0, mode="valid")[:n] * (0.05 + 0.1 * i)
        write_wav(os_join(root, f"bg/noise_{i}.wav"), noise, rate)
    return str(root)


def make_ir_db(root, lengths=(257, 1200, 4000), seed=1, rate=16000):
    """A directory of exponentially decaying noise impulse responses; returns the directory."""
    rng = np.random.RandomState(seed)
    for i, n in enumerate(lengths):
        ir = rng.randn(n) * np.exp(-np.arange(n) / (n / 6.0)) * 0.3
        ir[0] = 0.9
        write_wav(os_join(root, f"room_{i}.wav"), ir, rate)
    return str(root)


def os_join(root, rel):
    import os
    return os.path.join(str(root), rel)
