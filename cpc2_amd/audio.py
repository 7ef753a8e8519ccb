"""Audio file loading without torchaudio (absent from the image): FLAC through the native decoder of
libcpc2_hip.so (cpc_flac_decode_f32, MD5-verified), PCM / float WAV through a small RIFF parser.
`load(path)` returns what `torchaudio.load(path)[0]` returns: float32 [channels, samples] in [-1, 1)
(reference call sites: cpc/dataset.py:411-437, cpc/feature_loader.py:343).

Sample-rate conversion (`resample`, `resample_pack`) is torchaudio's sinc_interp_hann resampler on the device
(csrc/resample.hip; the definition is in include/cpc2_hip.h), and `save_wav` is the writer `load` reads back: PCM16 quantised on
the device, or IEEE float.  `pitch_shift` is the direct call of the `pitch_wsola` augmentation's kernels (csrc/pitch.hip), `freeverb`
that of the `freeverb` augmentation's kernel (csrc/freeverb.hip), `bandreject` that of the `bandreject_sinc` augmentation's
(csrc/bandreject.hip)."""
import collections
import ctypes
import struct

import numpy as np
import torch

from . import _lib


def info(path):
    """(sample_rate, channels, num_frames) -- torchaudio.info(...).num_frames of dataset.py:759-768."""
    path = str(path)
    if path.lower().endswith(".flac"):
        sr, ch, bps, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_long()
        _lib.check(_lib.load().cpc_flac_info(path.encode(), ctypes.byref(sr), ctypes.byref(ch), ctypes.byref(bps),
                                             ctypes.byref(n)), f"flac_info({path})")
        return sr.value, ch.value, n.value
    wav, sr = _load_wav(path, header_only=True)
    return sr, wav[0], wav[1]


def load(path):
    path = str(path)
    if path.lower().endswith(".flac"):
        sr, ch, n = info(path)
        out = torch.empty(ch, n, dtype=torch.float32)
        ok = ctypes.c_int()
        _lib.check(_lib.load().cpc_flac_decode_f32(path.encode(), _lib.ptr(out), out.numel(), ctypes.byref(ok)),
                   f"flac_decode({path})")
        return out, sr
    return _load_wav(path)


def _load_wav(path, header_only=False):
    with open(path, "rb") as f:
        data = f.read()
    if data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise ValueError(f"{path}: not a RIFF/WAVE file (only .flac and .wav are supported)")
    pos, fmt, payload = 12, None, None
    while pos + 8 <= len(data):
        tag, size = data[pos:pos + 4], struct.unpack_from("<I", data, pos + 4)[0]
        body = data[pos + 8:pos + 8 + size]
        if tag == b"fmt ":
            fmt = struct.unpack_from("<HHIIHH", body, 0)
        elif tag == b"data":
            payload = body
            break
        pos += 8 + size + (size & 1)
    if fmt is None or payload is None:
        raise ValueError(f"{path}: missing fmt/data chunk")
    code, channels, rate, _byte_rate, block_align, bits = fmt
    if code == 0xFFFE and len(data) > 0:          # WAVE_FORMAT_EXTENSIBLE: the real code follows
        code = 3 if bits == 32 and b"\x03\x00\x00\x00\x00\x00\x10\x00" in data[:128] else 1
    frames = len(payload) // block_align
    if header_only:
        return (channels, frames), rate
    if code == 1 and bits == 16:
        x = np.frombuffer(payload, dtype="<i2", count=frames * channels).astype(np.float32) / 32768.0
    elif code == 1 and bits == 8:
        x = (np.frombuffer(payload, dtype=np.uint8, count=frames * channels).astype(np.float32) - 128.0) / 128.0
    elif code == 1 and bits == 24:
        b = np.frombuffer(payload, dtype=np.uint8, count=frames * channels * 3).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        x = ((v ^ 0x800000) - 0x800000).astype(np.float32) / 8388608.0
    elif code == 1 and bits == 32:
        x = np.frombuffer(payload, dtype="<i4", count=frames * channels).astype(np.float32) / 2147483648.0
    elif code == 3 and bits == 32:
        x = np.frombuffer(payload, dtype="<f4", count=frames * channels).astype(np.float32)
    else:
        raise ValueError(f"{path}: unsupported WAV encoding (format {code}, {bits} bits)")
    return torch.from_numpy(x.reshape(frames, channels).T.copy()), rate


# --------------------------------------------------------------------------- sample-rate conversion
MAX_TABLE_FLOATS = 1 << 26          # 256 MB: rates with a small common divisor give n x (2 w + o) tables beyond any use
MAX_CACHED_TABLES = 8               # device tables kept, least recently used first out ...
MAX_CACHED_FLOATS = MAX_TABLE_FLOATS  # ... and never more floats of them than this beside the one in use
_tables = collections.OrderedDict()


def resample_plan(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """(o, n, w, taps) of a pair of rates: o input samples give n output samples through n phases of `taps` taps."""
    vals = [ctypes.c_int() for _ in range(4)]
    _lib.check(_lib.load().cpc_resample_plan(int(orig_freq), int(new_freq), int(lowpass_filter_width), float(rolloff),
                                             *[ctypes.byref(v) for v in vals]), "resample_plan")
    return tuple(v.value for v in vals)


def resample_table(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """The [n, taps] float32 table on the host (computed in double by the library, rounded once)."""
    o, n, w, taps = resample_plan(orig_freq, new_freq, lowpass_filter_width, rolloff)
    if n * taps > MAX_TABLE_FLOATS:
        raise ValueError(f"resampling {orig_freq} -> {new_freq} Hz reduces to {o} -> {n}: a table of {n} x {taps} taps; "
                         "choose rates with a larger common divisor")
    table = torch.empty(n, taps, dtype=torch.float32)
    _lib.check(_lib.load().cpc_resample_table_host(int(orig_freq), int(new_freq), int(lowpass_filter_width), float(rolloff),
                                                   _lib.ptr(table), table.numel()), "resample_table_host")
    return table


def output_length(length, o, n):
    return (n * int(length) + o - 1) // o


def _device_table(orig_freq, new_freq, lowpass_filter_width, rolloff, device):
    o, n, w, taps = resample_plan(orig_freq, new_freq, lowpass_filter_width, rolloff)
    key = (o, n, int(lowpass_filter_width), float(rolloff), device.type, device.index)
    table = _tables.pop(key, None)
    if table is None:
        table = resample_table(orig_freq, new_freq, lowpass_filter_width, rolloff).to(device)
    _tables[key] = table                                               # (most recently used last)
    def others():
        return sum(t.numel() for t in _tables.values()) - table.numel()

    while len(_tables) > 1 and (len(_tables) > MAX_CACHED_TABLES or others() > MAX_CACHED_FLOATS):
        _tables.popitem(last=False)
    return (o, n, w, taps), table


def _launch(flat, offsets, lengths, out, out_offsets, plan, table):
    o, n, w, _taps = plan
    device = flat.device
    tables = torch.tensor([list(offsets), list(lengths), list(out_offsets)], dtype=torch.int64).to(device)
    _lib.check(_lib.load().cpc_resample(_lib.ptr(flat), flat.numel(), _lib.ptr(tables[0]), _lib.ptr(tables[1]), len(lengths),
                                        max(lengths), _lib.ptr(table), o, n, w, _lib.ptr(out), out.numel(), _lib.ptr(tables[2]),
                                        _lib.stream_ptr(device)), "resample")


def resample(waveform, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """torchaudio.functional.resample(..., resampling_method="sinc_interp_hann"): [..., L] float32 on the device ->
    [..., ceil(n L / o)], every row on its own.  Equal rates return the input itself and launch nothing."""
    _lib.require_gpu(waveform)
    if int(orig_freq) == int(new_freq):
        return waveform
    x = _lib.f32c(waveform)
    plan, table = _device_table(orig_freq, new_freq, lowpass_filter_width, rolloff, x.device)
    length = x.shape[-1]
    rows = x.numel() // length if length else 0
    out_len = output_length(length, plan[0], plan[1])
    out = torch.empty(x.shape[:-1] + (out_len,), dtype=torch.float32, device=x.device)
    if rows and out_len:
        _launch(x.view(-1), [r * length for r in range(rows)], [length] * rows, out.view(-1), [r * out_len for r in range(rows)],
                plan, table)
    return out


def resample_pack(signals, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, lengths=None, offsets=None, out=None,
                  out_offsets=None):
    """Many signals, one launch.  `signals`: a list of 1-D float32 device tensors, or one flat vector with `lengths` (and
    `offsets` when the signals do not follow one another).  Returns a list of views of one flat output vector: signal i at
    out[out_offsets[i] .. + ceil(n lengths[i] / o)) -- `out` / `out_offsets` default to a dense vector; nothing else of a given
    `out` is written.  Each result has the bits `resample` gives the signal alone.  Equal rates: views of the input."""
    if isinstance(signals, (list, tuple)):
        if not signals:
            return []
        _lib.require_gpu(*signals)
        if any(s.dim() != 1 for s in signals):
            raise ValueError("resample_pack takes 1-D signals (or a flat vector with lengths)")
        lengths = [int(s.numel()) for s in signals]
        flat = torch.cat([_lib.f32c(s) for s in signals])
        offsets = None
    else:
        _lib.require_gpu(signals)
        if lengths is None:
            raise ValueError("a flat vector needs the signals' lengths")
        flat = _lib.f32c(signals).view(-1)
        lengths = [int(v) for v in lengths]
    if offsets is None:
        offsets = [0] * len(lengths)
        for i in range(1, len(lengths)):
            offsets[i] = offsets[i - 1] + lengths[i - 1]
    offsets = [int(v) for v in offsets]
    if len(offsets) != len(lengths) or any(v < 0 for v in lengths) or any(a < 0 or a + b > flat.numel() for a, b in zip(offsets, lengths)):
        raise ValueError("resample_pack: a signal leaves the flat vector")
    if int(orig_freq) == int(new_freq):
        return [flat[a:a + b] for a, b in zip(offsets, lengths)]
    plan, table = _device_table(orig_freq, new_freq, lowpass_filter_width, rolloff, flat.device)
    out_lens = [output_length(v, plan[0], plan[1]) for v in lengths]
    if out_offsets is None:
        out_offsets = [0] * len(out_lens)
        for i in range(1, len(out_lens)):
            out_offsets[i] = out_offsets[i - 1] + out_lens[i - 1]
    out_offsets = [int(v) for v in out_offsets]
    if out is None:
        out = torch.empty(max(a + b for a, b in zip(out_offsets, out_lens)), dtype=torch.float32, device=flat.device)
    else:
        _lib.require_gpu(out)
        if out.dtype != torch.float32 or not out.is_contiguous() or out.dim() != 1 or out.device != flat.device:
            raise TypeError("resample_pack: out is a contiguous 1-D float32 vector on the signals' device")
    if len(out_offsets) != len(out_lens) or any(a < 0 or a + b > out.numel() for a, b in zip(out_offsets, out_lens)):
        raise ValueError("resample_pack: a result leaves the output vector")
    if flat.numel() and out.numel() and max(lengths) > 0:
        _launch(flat, offsets, lengths, out, out_offsets, plan, table)
    return [out[a:a + b] for a, b in zip(out_offsets, out_lens)]


# --------------------------------------------------------------------------- pitch shift
def pitch_shift(x, cents, return_offsets=False):
    """The `pitch_wsola` pitch shift (data_augmentation.PitchShiftAugment states it; csrc/pitch.hip) of [..., W] float32 device
    rows sampled at 16 kHz: `cents` is one int for all rows or one value per row, each within +-1200; 0 returns the row's bits.
    The result has x's shape.  return_offsets: also the segment starts the search chose, [rows, J] int32 on the device.  This is
    this package's definition of a pitch shift, not sox's; nothing is drawn here."""
    from . import data_augmentation as da
    _lib.require_gpu(x)
    x = _lib.f32c(x)
    window = x.shape[-1]
    rows = x.numel() // window if window else 0
    per_row = np.asarray(cents.cpu() if isinstance(cents, torch.Tensor) else cents)
    if per_row.dtype.kind not in "iu":
        raise TypeError("pitch_shift: cents are whole numbers (an int, or one per row)")
    if per_row.ndim == 0:
        per_row = np.full(rows, int(per_row), dtype=np.int64)
    if per_row.size != rows:
        raise ValueError(f"pitch_shift: {per_row.size} values of cents for {rows} rows")
    out = torch.empty_like(x)
    if rows == 0:
        return (out, torch.empty(0, 1, dtype=torch.int32, device=x.device)) if return_offsets else out
    tables = da.pitch_tables(per_row, window)
    dev = {k: torch.from_numpy(tables[k]).to(x.device) for k in ("cents", "ratio", "cutoff", "nominal")}
    q = da._pitch_launch(x.view(rows, window), dev, 0, rows, tables["cents_bound"], window, out.view(rows, window), "pitch_shift")
    return (out, q) if return_offsets else out


# --------------------------------------------------------------------------- artificial reverberation
def freeverb(x, room, reverberance=100.0, hf_damping=100.0, wet_gain_dB=0.0):
    """The `freeverb` reverberation (data_augmentation.FreeverbAugment states it; csrc/freeverb.hip) of [b, 1, W], [b, W] or [W]
    float32 device rows sampled at 16 kHz: `room` is one room size (0 to 100) for all rows or one per row.  The result has x's
    shape.  This is this package's statement of the Freeverb network, not sox's `reverb`; nothing is drawn here."""
    from . import data_augmentation as da
    _lib.require_gpu(x)
    x = _lib.f32c(x)
    window = x.shape[-1]
    rows = x.numel() // window if window else 0
    per_row = np.asarray(room.cpu() if isinstance(room, torch.Tensor) else room)
    if per_row.dtype.kind not in "iu":
        raise TypeError("freeverb: room sizes are whole numbers (an int, or one per row)")
    if per_row.ndim == 0:
        per_row = np.full(rows, int(per_row), dtype=np.int64)
    if per_row.size != rows:
        raise ValueError(f"freeverb: {per_row.size} room sizes for {rows} rows")
    tables = da.freeverb_tables(per_row, reverberance, hf_damping, wet_gain_dB)
    out = torch.empty_like(x)
    if rows == 0:
        return out
    comb_len = torch.from_numpy(tables["comb_len"]).to(x.device)
    da._freeverb_launch(x.view(rows, window), comb_len, 0, rows, tables, window, out.view(rows, window), "freeverb")
    return out


# --------------------------------------------------------------------------- band reject
def bandreject(x, low, high, attenuation_dB=120.0, transition_hz=400.0):
    """The `bandreject_sinc` filter (data_augmentation.BandrejectSincAugment states it; csrc/bandreject.hip) of [b, 1, W], [b, W] or
    [W] float32 device rows sampled at 16 kHz: the band `low` .. `high` in Hz (0 <= low <= high <= 8000) is one pair for all rows
    or one per row.  The result has x's shape.  This is this package's Kaiser-windowed sinc filter, not sox's `sinc`; nothing is
    drawn here and there is no dither."""
    from . import data_augmentation as da
    _lib.require_gpu(x)
    x = _lib.f32c(x)
    window = x.shape[-1]
    rows = x.numel() // window if window else 0
    edges = []
    for name, value in (("low", low), ("high", high)):
        per_row = np.asarray(value.cpu() if isinstance(value, torch.Tensor) else value, dtype=np.float64)
        if per_row.ndim == 0:
            per_row = np.full(rows, float(per_row), dtype=np.float64)
        if per_row.size != rows:
            raise ValueError(f"bandreject: {per_row.size} {name} edges for {rows} rows")
        edges.append(per_row.reshape(-1))
    tables = da.bandreject_tables(edges[0], edges[1], attenuation_dB, transition_hz)
    out = torch.empty_like(x)
    if rows == 0:
        return out
    band = torch.from_numpy(tables["band"]).to(x.device)
    da._bandreject_launch(x.view(rows, window), band, 0, rows, tables, window, out.view(rows, window), "bandreject")
    return out


def to_pcm16(waveform):
    """(int16 tensor of the same shape, device counter of clamped samples): q = clamp(rint(32768 y), -32768, 32767), the
    inverse of what reading a PCM16 file does.  Nothing is synchronised."""
    _lib.require_gpu(waveform)
    y = _lib.f32c(waveform)
    q = torch.empty(y.shape, dtype=torch.int16, device=y.device)
    clamped = torch.zeros(1, dtype=torch.int64, device=y.device)
    _lib.check(_lib.load().cpc_resample_to_pcm16(_lib.ptr(y), y.numel(), _lib.ptr(q), _lib.ptr(clamped), _lib.stream_ptr(y.device)),
               "resample_to_pcm16")
    return q, clamped


def write_wav(path, samples, rate):
    """RIFF/WAVE from HOST samples [channels, frames]: int16 -> PCM16, float32 -> IEEE float (format 3)."""
    a = samples.numpy() if isinstance(samples, torch.Tensor) else np.asarray(samples)
    if a.ndim != 2 or a.dtype not in (np.int16, np.float32):
        raise TypeError("write_wav takes [channels, frames] int16 or float32 samples")
    channels, frames = a.shape
    code, bits = (1, 16) if a.dtype == np.int16 else (3, 32)
    block = channels * bits // 8
    payload = np.ascontiguousarray(a.T).astype("<i2" if code == 1 else "<f4", copy=False).tobytes()
    if len(payload) + 36 >= 1 << 32:
        raise ValueError(f"{path}: {len(payload)} bytes of samples do not fit a RIFF file")
    header = b"RIFF" + struct.pack("<I", 36 + len(payload)) + b"WAVE" + b"fmt " + struct.pack(
        "<IHHIIHH", 16, code, channels, int(rate), int(rate) * block, block, bits) + b"data" + struct.pack("<I", len(payload))
    with open(path, "wb") as f:
        f.write(header)
        f.write(payload)


def save_wav(path, waveform, rate, precision=16):
    """torchaudio.save(path, waveform, rate, precision=..., channels_first=True) for .wav: [channels, samples] float32.
    precision 16: PCM16, quantised on the device (a device tensor is required); 32: IEEE float, from either side.
    Returns the number of samples the PCM16 clamp changed (0 for float)."""
    if waveform.dim() != 2:
        raise ValueError("save_wav takes a [channels, samples] tensor")
    if precision == 32:
        if waveform.dtype != torch.float32:
            raise TypeError(f"save_wav writes float32 samples (got {waveform.dtype})")
        write_wav(path, waveform.detach().cpu(), rate)
        return 0
    if precision != 16:
        raise ValueError(f"save_wav writes 16-bit PCM or 32-bit float, not precision={precision}")
    q, clamped = to_pcm16(waveform)
    write_wav(path, q.cpu(), rate)
    return int(clamped.item())
