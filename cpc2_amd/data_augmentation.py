"""Audio augmentation on device batches: the reference's cpc/data_augmentation.py for the types whose arithmetic is fixed.

Built: `additive` (AdditiveNoiseAugment :157-228), `natural_reverb` (NaturalReverb :278-318), `time_dropout`
(TimeDropoutAugment :268-275), `pitch_wsola` (PitchShiftAugment: a pitch shift by this package's own definition, below),
`freeverb` (FreeverbAugment: artificial reverberation by this package's own definition, below), `bandreject_sinc`
(BandrejectSincAugment: a band-reject filter by this package's own definition, below), their
combinations (CombinedTransforms :331-344) and the reverberated noise (`augmentation_factory(..., applied_on_noise=True)`).
The sox types (UNBUILT_TYPES: pitch, pitch_quick, pitch_dropout, pitch_deropout, bandreject, artificial_reverb, ...) are refused
by name: neither sox nor WavAugment is available, and their filters cannot be pinned to anything.  `pitch_wsola` is NOT one of
them under another name: it draws what the reference's PitchAugment draws and shifts the pitch, by an algorithm written down in
PitchShiftAugment's docstring; its agreement with sox's `pitch` effect is unmeasured.  `--augment_type pitch_wsola time_dropout`
stands in for the reference's `pitch_dropout`.  `freeverb` likewise: it draws what the reference's ReverbAugment draws (one room
size per window) and reverberates with the public-domain Freeverb network -- the algorithm behind sox's `reverb` -- as written down
in FreeverbAugment's docstring; `artificial_reverb` and `artificial_reverb_dropout` stay refused, the agreement of `freeverb` with
sox's output is unmeasured, and `--augment_type freeverb time_dropout` stands in for `artificial_reverb_dropout`.
`bandreject_sinc` likewise: it draws what the reference's BandrejectAugment draws (one band per window on the mel scale) and
rejects the band with a Kaiser-windowed sinc FIR -- the textbook filter behind sox's `sinc -a 120 high-low` -- as written down in
BandrejectSincAugment's docstring; `bandreject` itself stays refused and the agreement with sox's output is unmeasured.

The reference augments one window at a time on the CPU, inside DataLoader workers.  Here a pack of audio lives in HBM as one
flat vector and so do the noise pack and the impulse responses; a batch's augmentation is a few kernels
(csrc/augment.hip) that read the windows by offset, and the host only draws numbers -- once per pack:

  * a transform draws ONE window's numbers with `draw_one(window)` (an "entry"), in the order the reference's `__call__` draws
    them and from the same generators -- numpy's global generator for the SNR, the dropout's two integers and the
    impulse_response_prob test; Python's `random` for the impulse-response choice; the noise loader's samplers draw from
    `random` and torch's generator;
  * `seal(entries, device)` turns a list of entries into a PLAN: a dict of host numpy arrays (what the tests replay through the
    fp64 statement of the transforms) plus, under "_dev", the same arrays on the device (one pinned, non-blocking copy each);
  * `apply(plan, lo, hi, src, dst=None, window=None)` augments the windows `src` with rows [lo, hi) of the plan; a step of the training loop
    uploads nothing and waits for nothing.  `src` is a [b, 1, W] / [b, W] device buffer or FlatWindows(vector, offsets).

`transform(x)` on a [b, 1, W] device batch or on the reference's single [1, W] window draws, seals and applies in one go; the
plan it used stays in `transform.last_plan`.

Deviations from the reference, all deliberate:
  * impulse responses are never resampled: a file whose rate is not `sr` is refused with an error that names it;
  * sequence-wise NaturalReverb: the probability test is drawn from numpy and the file from `random` (the reference's library
    draws both from torch); a file is drawn only for a window the test lets through;
  * TimeDropoutAugment follows the definition in its docstring (the library the reference calls is not available);
  * PitchShiftAugment likewise: a WSOLA stretch and a windowed-sinc resampling instead of sox's pitch / rate chain, no dither;
  * FreeverbAugment: one mono bank of eight combs and four all-passes at 16 kHz instead of sox's `reverb` chain: no pre-delay, no
    tone filters, no stereo spread, no dither, no clipping, no peak normalisation, and the tail beyond the window is cut off (as
    natural_reverb cuts it);
  * BandrejectSincAugment: a Kaiser-windowed sinc FIR of this package's design instead of sox's `sinc` / `dither` chain: no
    dither, no clipping, no peak normalisation, zeros outside the window;
  * `--augment_type none` gives None (the reference's factory raises on the one-element list ['none']).
"""
import collections
import ctypes
import os
import random

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr

BUILT_TYPES = ('additive', 'natural_reverb', 'time_dropout', 'pitch_wsola')
OWN_TYPES = ('freeverb',)              # built as well; a tuple of its own, listed after BUILT_TYPES wherever the types are named
FILTER_TYPES = ('bandreject_sinc',)   # built as well; a third tuple, named before BUILT_TYPES wherever the types are listed
UNBUILT_TYPES = ('bandreject', 'pitch', 'pitch_quick', 'pitch_dropout', 'pitch_deropout', 'artificial_reverb',
                 'artificial_reverb_dropout', 'random_noise')

energy_normalization = lambda wav: wav / (torch.sqrt(torch.mean(wav ** 2)) + 1e-8)                  # noqa: E731
peak_normalization = lambda wav: wav / (wav.abs().max(dim=1, keepdim=True)[0] + 1e-8)              # noqa: E731

FlatWindows = collections.namedtuple("FlatWindows", "data offsets")     # windows data[offsets[i] : offsets[i] + W] (device tensors)


def unbuilt_message(augment_type):
    """The refusal of a request that names a type without a kernel path (train.refuseUnsupported, augmentation_factory)."""
    asked = [augment_type] if isinstance(augment_type, str) else list(augment_type)
    missing = [t for t in asked if t not in BUILT_TYPES + OWN_TYPES + FILTER_TYPES and t != 'none']
    return (f"--augment_past / --augment_future with --augment_type {' '.join(asked)}: {', '.join(missing)} "
            f"{'is' if len(missing) == 1 else 'are'} not built (sox / WavAugment effects); the augmentation types on the MI355X "
            f"feeder path are {', '.join(FILTER_TYPES + BUILT_TYPES)}, {', '.join(OWN_TYPES)} and none, alone or combined")


# --------------------------------------------------------------------------- device helpers
def _upload(array, device):
    """A host array on the device through one pinned, asynchronous copy (nothing waits for it)."""
    t = torch.from_numpy(np.ascontiguousarray(array))
    if device.type != "cuda":
        return t
    return t.pin_memory().to(device, non_blocking=True)


def _rows(t):
    return t.reshape(-1, t.shape[-1])


def _operand(src):
    """(pointer, total, offsets pointer) of a kernel operand: FlatWindows or a contiguous buffer."""
    if isinstance(src, FlatWindows):
        return ptr(src.data), src.data.numel(), ptr(src.offsets)
    return ptr(src), 0, ptr(None)


def _count(src):
    return src.offsets.numel() if isinstance(src, FlatWindows) else _rows(src).size(0)


def _device_of(src):
    return src.data.device if isinstance(src, FlatWindows) else src.device


def _buffer(src, window, dst=None):
    """`src` as a [b, W] buffer: itself, or its windows gathered into dst (a new buffer when None)."""
    if not isinstance(src, FlatWindows):
        return src
    b = src.offsets.numel()
    out = dst if dst is not None else torch.empty(b, window, dtype=torch.float32, device=src.data.device)
    check(_lib.load().cpc_window_gather(ptr(src.data), src.data.numel(), ptr(src.offsets), ptr(out), b, window,
                                        stream_ptr(src.data.device)), "window_gather")
    return out


def _window(src, dst, window=None):
    """Samples per window: of the buffer operand, of dst, or as told (windows given by offsets carry no length)."""
    if not isinstance(src, FlatWindows):
        return src.shape[-1]
    if dst is not None:
        return dst.shape[-1]
    if window is None:
        raise ValueError("windows given by offsets need dst or window")
    return window


def _check_src(src):
    if isinstance(src, FlatWindows):
        _lib.require_gpu(src.data, src.offsets)
        if src.data.dtype != torch.float32 or src.offsets.dtype != torch.int64 or not src.offsets.is_contiguous():
            raise TypeError("FlatWindows needs a float32 vector and contiguous int64 offsets")
    else:
        _lib.require_gpu(src)
        if src.dtype != torch.float32 or not src.is_contiguous():
            raise TypeError("augmentation kernels take contiguous float32 batches")


def peak_norm_windows(src, window, dst=None):
    """PeakNorm (cpc/dataset.py:433-438) of every window of `src`, on the device: w / (max|w| + 1e-8)."""
    _check_src(src)
    b, dev = _count(src), _device_of(src)
    out = dst if dst is not None else torch.empty(b, window, dtype=torch.float32, device=dev)
    p, total, off = _operand(src)
    check(_lib.load().cpc_augment_peak_norm(p, total, off, ptr(out), b, window, stream_ptr(dev)), "augment_peak_norm")
    return out


class _Transform:
    """What the built transforms share: draw / seal / apply (module docstring) and the reference's `__call__`."""
    inplace = False

    def plan(self, n, window, device):
        return self.seal([self.draw_one(window) for _ in range(n)], torch.device(device))

    def __call__(self, x):
        _lib.require_gpu(x)
        window = x.shape[-1]
        rows = _rows(x.contiguous())
        plan = self.plan(rows.size(0), window, x.device)
        self.last_plan = plan
        src = rows.clone() if self.inplace else rows
        return _rows(self.apply(plan, 0, rows.size(0), src)).view(x.shape)


# --------------------------------------------------------------------------- additive noise
class AdditiveNoiseAugment(_Transform):
    """data_augmentation.py:157-228.  Per window: the next window of the noise data set (after its PeakNorm transform and, with
    meta-augmentation, its own augmentation), snr = (snr_max - snr_min) u + snr_min with u one np.random.random_sample(),
    g = 10 ** (-snr / 20), and peak_normalization(energy_normalization(x) + energy_normalization(noise) * g).

    Noise windows are taken as the reference takes them (:176-211): a loader of batchSize windows over all packs of the noise
    data set -- `uniform`, or `temporalsamespeaker` with remove_artefacts -- with a random offset, consumed one window per
    call and started again when it runs out.  The first noise batch is fetched when the transform is built, as there.  When a
    noise batch is fetched and the noise data set carries an augmentation (`--meta_aug`), that augmentation's numbers for the
    batch's windows are drawn right then.

    Entry: (noise vector, noise offset, meta entry or None, snr).  Plan: snr [n] f64, gain [n] f32, noise_off [n] i64,
    noise_src [n] (index into noise_data, the device vectors the offsets refer to), meta (the noise augmentation's plan)."""

    def __init__(self, noise_dataset, snr_min, snr_max, batchSize, sampling='uniform'):
        assert noise_dataset and snr_min <= snr_max
        self.noise_dataset = noise_dataset
        self.sampling = sampling
        self.batchSize = batchSize
        self.snr_min = snr_min
        self.snr_max = snr_max
        self.meta = noise_dataset.augmentation if getattr(noise_dataset, "augment_past", False) else None
        self.peak_norm = getattr(noise_dataset, "transform", None) is not None
        self.current_noise_batch = collections.deque()
        self.update_noise_loader()
        self.get_next_batch()

    def update_noise_loader(self):
        loader = self.noise_dataset.getDataLoader(self.batchSize, type=self.sampling, randomOffset=True, numWorkers=0,
                                                  onLoop=-1, nLoops=-1, remove_artefacts=self.sampling != "uniform")
        self.noise_data_loader = loader.offsets()

    def get_next_batch(self):
        try:
            data, batch = next(self.noise_data_loader)
        except StopIteration:
            self.update_noise_loader()
            try:
                data, batch = next(self.noise_data_loader)
            except StopIteration:
                raise RuntimeError("the noise data set yields no window (is it shorter than a batch of windows?)")
        window = self.noise_dataset.sizeWindow
        self.current_noise_batch = collections.deque(
            (data, int(o), self.meta.draw_one(window) if self.meta is not None else None) for o in batch)

    def get_noise_sequence(self):
        if not self.current_noise_batch:
            self.get_next_batch()
        return self.current_noise_batch.popleft()

    def draw_one(self, window):
        data, offset, meta = self.get_noise_sequence()
        snr = (self.snr_max - self.snr_min) * np.random.random_sample() + self.snr_min
        return data, offset, meta, snr

    def seal(self, entries, device):
        tensors, index = [], {}
        src = np.empty(len(entries), dtype=np.int64)
        for i, (data, _o, _m, _s) in enumerate(entries):
            key = id(data)
            if key not in index:
                index[key] = len(tensors)
                tensors.append(data)
            src[i] = index[key]
        snr = np.array([e[3] for e in entries], dtype=np.float64)
        gain = (1.0 / (10.0 ** (snr / 20.0))).astype(np.float32)               # :219-220, a = snr / 20, 1 / 10 ** a
        plan = {"kind": "additive", "n": len(entries), "snr": snr, "gain": gain,
                "noise_off": np.array([e[1] for e in entries], dtype=np.int64), "noise_src": src, "noise_data": tensors,
                "noise_peak_norm": self.peak_norm,
                "meta": self.meta.seal([e[2] for e in entries], device) if self.meta is not None else None}
        plan["_dev"] = {"gain": _upload(gain, device), "noise_off": _upload(plan["noise_off"], device)}
        return plan

    @staticmethod
    def _runs(plan, lo, hi):
        """[lo, hi) cut where the noise vector changes (a noise data set of several packs); almost always one run."""
        if len(plan["noise_data"]) == 1:
            return [(lo, hi, plan["noise_data"][0])]
        src = plan["noise_src"][lo:hi]
        cuts = [0] + (np.flatnonzero(np.diff(src)) + 1).tolist() + [hi - lo]
        return [(lo + a, lo + b, plan["noise_data"][int(src[a])]) for a, b in zip(cuts[:-1], cuts[1:])]

    def apply(self, plan, lo, hi, src, dst=None, window=None):
        _check_src(src)
        lib, dev = _lib.load(), _device_of(src)
        b = hi - lo
        window = _window(src, dst, window if window is not None else self.noise_dataset.sizeWindow)
        out = dst if dst is not None else torch.empty(b, window, dtype=torch.float32, device=dev)
        d = plan["_dev"]
        for a, e, noise in self._runs(plan, lo, hi):
            noise_src = FlatWindows(noise, d["noise_off"][a:e])
            peak = 1 if plan["noise_peak_norm"] else 0
            if plan["meta"] is not None:
                # the noise window as the noise data set yields it: PeakNorm, then its own augmentation
                clean = peak_norm_windows(noise_src, window) if peak else _buffer(noise_src, window)
                noise_src, peak = self.meta.apply(plan["meta"], a, e, clean), 0
            if isinstance(src, FlatWindows):
                part = FlatWindows(src.data, src.offsets[a - lo:e - lo])
            else:
                part = _rows(src)[a - lo:e - lo]
            sp, st, so = _operand(part)
            np_, nt, no = _operand(noise_src)
            check(lib.cpc_augment_additive(sp, st, so, np_, nt, no, peak, ptr(d["gain"][a:e]), ptr(_rows(out)[a - lo:e - lo]),
                                           e - a, window, stream_ptr(dev)), "augment_additive")
        return out


# --------------------------------------------------------------------------- natural reverberation
class NaturalReverb(_Transform):
    """data_augmentation.py:278-318: y[t] = sum_{k <= t} ir[k] x[t - k] for t < W (the convolution cut to the input length, no
    delay compensation), then peak_normalization.  With probability 1 - p the convolution is skipped; the normalisation is
    applied either way.  Sequence-wise (default): every window draws its own impulse response; batch_wise: one response serves
    batchSize consecutive windows, then a new one is drawn (:312-317; the first one when the transform is built).

    The responses are the .wav files under ir_paths (findAllSeqs, no cache), mixed to mono and loaded once to the device as one
    flat vector with an offsets table.  A file whose rate is not `sr` is refused: nothing is resampled here
    (cpc2_amd.eval.utils.adjust_sample_rate converts a directory beforehand).

    Entry: index of the response, or -1 for a skipped convolution.  Plan: ir_index [n] i64, ir_off [n] i64, ir_len [n] i32."""

    def __init__(self, ir_paths, p, batchSize, sr=32000, batch_wise=False, device=None):
        from . import audio
        from .dataset import findAllSeqs
        self.p = p
        self.sr = sr
        self.batch_wise = batch_wise
        self.count = 0
        self.batchSize = batchSize
        if ir_paths is None:
            raise ValueError("natural_reverb needs --pathImpulseResponses")
        files, _ = findAllSeqs(ir_paths, extension=".wav")
        self.ir_files = [os.path.join(ir_paths, data[1]) for data in files]
        print("Found %d files for natural reverberation" % len(self.ir_files))
        if not self.ir_files:
            raise ValueError(f"no .wav impulse response under {ir_paths}")
        responses = []
        for path in self.ir_files:
            wav, rate = audio.load(path)
            if rate != sr:
                raise ValueError(f"impulse response {path} is sampled at {rate} Hz, not at --ir_sample_rate {sr}: responses "
                                 "are not resampled here, convert the file.  `python -m cpc2_amd.eval.utils.adjust_sample_rate "
                                 f"{ir_paths} OUT_DIR --out_sample_rate {sr} --recursive` converts the whole directory")
            responses.append(wav.float().mean(dim=0))
        self.ir_len = np.array([r.numel() for r in responses], dtype=np.int64)
        self.ir_off = np.concatenate([[0], np.cumsum(self.ir_len)[:-1]]).astype(np.int64)
        self.device = torch.device(device) if device is not None else \
            torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.ir_data = torch.cat(responses).to(self.device)
        if batch_wise:
            self.get_new_impulse_response()

    def get_new_impulse_response(self):
        self.current = random.choice(range(len(self.ir_files)))

    def draw_one(self, window):
        applied = np.random.random_sample() < self.p
        if self.batch_wise:
            index = self.current if applied else -1
            self.count += 1
            if self.count == self.batchSize:
                self.get_new_impulse_response()
                self.count = 0
            return index
        return random.choice(range(len(self.ir_files))) if applied else -1

    def seal(self, entries, device):
        index = np.array(entries, dtype=np.int64).reshape(-1)
        safe = np.maximum(index, 0)
        plan = {"kind": "natural_reverb", "n": len(index), "ir_index": index,
                "ir_off": np.where(index >= 0, self.ir_off[safe], 0).astype(np.int64),
                "ir_len": np.where(index >= 0, self.ir_len[safe], 0).astype(np.int32)}
        plan["_dev"] = {"ir_off": _upload(plan["ir_off"], device), "ir_len": _upload(plan["ir_len"], device)}
        return plan

    def apply(self, plan, lo, hi, src, dst=None, window=None):
        _check_src(src)
        lib, dev = _lib.load(), _device_of(src)
        b = hi - lo
        window = _window(src, dst, window)
        src = _buffer(src, window)
        out = dst if dst is not None else torch.empty(b, window, dtype=torch.float32, device=dev)
        need = lib.cpc_augment_fir_scratch_bytes(b, window)
        scratch = _lib.scratch(need, dev, tag="augment_fir")
        d = plan["_dev"]
        check(lib.cpc_augment_fir(ptr(src), ptr(self.ir_data), self.ir_data.numel(), ptr(d["ir_off"][lo:hi]),
                                  ptr(d["ir_len"][lo:hi]), ptr(out), ptr(scratch), scratch.numel(), b, window, stream_ptr(dev)),
              "augment_fir")
        return out


# --------------------------------------------------------------------------- time dropout
class TimeDropoutAugment(_Transform):
    """data_augmentation.py:268-275, by this definition: max_frames = int(sr * T_ms / 1000); per window
    length = np.random.randint(0, max_frames), then start = np.random.randint(0, max(1, W - length)); samples
    [start, start + length) become zero and every other sample is untouched, bit for bit.  T_ms below one sample's worth
    (max_frames == 0) is refused here.  In place.

    Entry: (start, length).  Plan: start [n] i64, length [n] i64."""
    inplace = True

    def __init__(self, T_ms=100, sr=16000.0):
        self.sr = sr
        self.max_frames = int(sr * T_ms / 1000)
        if self.max_frames <= 0:
            raise ValueError(f"--t_ms {T_ms}: a dropout of at most {self.max_frames} samples; give at least 1 ms")

    def draw_one(self, window):
        length = int(np.random.randint(0, self.max_frames))
        start = int(np.random.randint(0, max(1, window - length)))
        return start, length

    def seal(self, entries, device):
        arr = np.array(entries, dtype=np.int64).reshape(-1, 2)
        plan = {"kind": "time_dropout", "n": len(arr), "start": arr[:, 0].copy(), "length": arr[:, 1].copy()}
        plan["_dev"] = {"start": _upload(plan["start"], device), "length": _upload(plan["length"], device)}
        return plan

    def apply(self, plan, lo, hi, src, dst=None, window=None):
        _check_src(src)
        dev = _device_of(src)
        src = _buffer(src, _window(src, dst, window), dst)
        d = plan["_dev"]
        check(_lib.load().cpc_augment_time_dropout(ptr(src), ptr(d["start"][lo:hi]), ptr(d["length"][lo:hi]), hi - lo,
                                                   src.shape[-1], stream_ptr(dev)), "augment_time_dropout")
        return src


# --------------------------------------------------------------------------- pitch shift
PITCH_SEGMENT, PITCH_OVERLAP, PITCH_SEARCH = 1312, 192, 234          # S, O, R in samples at 16 kHz: 82 ms, 12 ms, 14.68 ms
PITCH_HOP = PITCH_SEGMENT - PITCH_OVERLAP                            # Ho, the output hop
PITCH_SINC_WIDTH, PITCH_ROLLOFF = 6, 0.99                            # L and the low-pass cutoff factor
PITCH_TAP_GUARD = 16                                                 # stretched samples allowed for beyond ceil(W r): > L / c - r
PITCH_MAX_CENTS = 1200


def pitch_segments(window, ratio):
    """J(W, r): segments of Ho stretched samples that cover every tap of every output, ceil((ceil(W r) + 16) / Ho)."""
    reach = int(np.ceil(window * ratio)) + PITCH_TAP_GUARD
    return -(-reach // PITCH_HOP)


def pitch_tables(cents, window, segments=None):
    """The host tables of a batch of shifts (PitchShiftAugment's docstring): cents [n] i32, ratio [n] f64 (C's pow(2, cents / 1200)
    in double), cutoff [n] f64, nominal [n, J] i32 with nominal[i, j] = floor(j Ho / ratio[i] + 0.5) and J the largest segment
    count of the batch (or `segments` when that is larger)."""
    cents = np.asarray(cents, dtype=np.int64).reshape(-1)
    if cents.size and int(np.abs(cents).max()) > PITCH_MAX_CENTS:
        raise ValueError(f"a pitch shift of {int(np.abs(cents).max())} cents: at most {PITCH_MAX_CENTS} (an octave) either way")
    ratio = np.array([2.0 ** (int(c) / 1200.0) for c in cents], dtype=np.float64)
    cutoff = PITCH_ROLLOFF * np.minimum(1.0, 1.0 / ratio)
    reach = np.ceil(window * ratio).astype(np.int64) + PITCH_TAP_GUARD                  # pitch_segments, all rows at once
    count = max([int((-(-reach // PITCH_HOP)).max()) if cents.size else 1, 1, int(segments or 1)])
    nominal = np.floor(np.arange(count, dtype=np.float64)[None, :] * PITCH_HOP / ratio[:, None] + 0.5)
    if nominal.size and nominal.max() + PITCH_SEARCH + PITCH_SEGMENT >= 2 ** 31:
        raise ValueError(f"windows of {window} samples: the segment starts of a pitch shift no longer fit 32 bits")
    return {"cents": cents.astype(np.int32), "ratio": ratio, "cutoff": cutoff, "nominal": nominal.astype(np.int32),
            "cents_bound": int(np.abs(cents).max()) if cents.size else 0}


def _pitch_launch(src, dev_tables, lo, hi, bound, window, out, what="augment_pitch"):
    """cpc_augment_pitch on rows [lo, hi) of device tables; returns the chosen segment starts [b, J] (int32)."""
    dev = _device_of(src)
    nominal = dev_tables["nominal"]
    q = torch.empty(hi - lo, nominal.shape[1], dtype=torch.int32, device=dev)
    p, total, off = _operand(src)
    check(_lib.load().cpc_augment_pitch(p, total, off, ptr(dev_tables["ratio"][lo:hi]), ptr(dev_tables["cutoff"][lo:hi]),
                                        ptr(dev_tables["cents"][lo:hi]), int(bound), ptr(nominal[lo:hi]), nominal.shape[1],
                                        ptr(out), ptr(q), hi - lo, window, stream_ptr(dev)), what)
    return q


class PitchShiftAugment(_Transform):
    """`pitch_wsola`: a pitch shift of every window by a whole number of cents, drawn as the reference's PitchAugment
    (data_augmentation.py:64-100) draws it -- ONE np.random.randint(-shift_max, shift_max) per window from numpy's global
    generator; the output has the input's length and is not peak-normalised.  The reference hands the number to a sox effect chain
    (pitch + rate + dither) that is not available; what happens to the window here is THIS PACKAGE'S definition, written down
    below.  It is not sox's algorithm, there is no dither, and its agreement with sox is unmeasured.  The constants are in samples
    and mean what they say at 16 kHz only; the three times are this package's choice (what sox `tempo`'s defaults are recalled to be,
    which could not be checked).

      S = 1312 (segment, 82 ms)   O = 192 (overlap, 12 ms)   R = 234 (search candidates, 14.68 ms)   Ho = S - O = 1120
      L = 6 (sinc half-width in zero crossings)   rolloff = 0.99

    The window x[0 .. W) is f32 and reads as zero outside [0, W), whatever lies beside it in a pack.  r = 2 ** (cents / 1200) in
    f64 on the host.  cents == 0 returns the window bit for bit.  Otherwise:

    Stage 1, a time stretch by r (WSOLA), stated as a function s(m), m >= 0.  Segment j = m // Ho, k = m - j Ho.
      q_0 = 0.  For j >= 1 the nominal start is p_j = floor(j Ho / r + 0.5) (f64, a host table), the template is
      t[k] = x[q_{j-1} + Ho + k], k < O (raw input: the tail of the previous segment), the candidates are p_j - R // 2 + d,
      d = 0 .. R - 1, and a candidate's cost is D(d) = sum_{k < O} (x[cand + k] - t[k]) ** 2, in f64: both values converted, the
      difference, its square, added with k ascending, nothing contracted.  q_j is the candidate of the smallest D, the lowest d on
      a tie.
      s(m) = x[q_j + k] for k >= O or j == 0; otherwise a + (k / O) (b - a) with a = x[q_{j-1} + Ho + k], b = x[q_j + k].
    Stage 2, resampling by r.  y[n] = sum_{m >= 0} h(n r - m) s(m) for n in [0, W), with c = 0.99 min(1, 1 / r) and
      h(t) = c sinc(c t) cos(pi c t / (2 L)) ** 2 for |c t| < L, else 0 (sinc(u) = sin(pi u) / (pi u)).

    On the device (csrc/pitch.hip) the q_j are the statement's, exactly; the weights are evaluated in f64 and rounded once to f32,
    the cross-fade likewise, and the sum is one f32 fmaf chain with m ascending, so a window's bits depend on nothing else in the
    batch or the pack.  J = ceil((ceil(W r) + 16) / Ho) segments cover every tap.

    Entry: cents.  Plan: cents [n] i32, ratio [n] f64, cutoff [n] f64, nominal [n, J] i32, window, cents_bound.  Out of place; the
    starts the last `apply` chose stay in `last_offsets` ([b, J] int32 on the device)."""

    def __init__(self, shift_max=300):
        if shift_max != int(shift_max):
            raise ValueError(f"--shift_max {shift_max}: pitch_wsola shifts by a whole number of cents")
        if shift_max < 1:
            raise ValueError(f"--shift_max {shift_max}: pitch_wsola draws from [-shift_max, shift_max) and needs at least 1 cent")
        if shift_max > PITCH_MAX_CENTS:
            raise ValueError(f"--shift_max {shift_max}: pitch_wsola shifts by at most {PITCH_MAX_CENTS} cents (an octave) either way")
        self.shift_max = int(shift_max)
        self.window = None
        self.last_offsets = None

    def draw_one(self, window):
        self.window = window
        return int(np.random.randint(-self.shift_max, self.shift_max))

    def seal(self, entries, device, window=None):
        window = window if window is not None else self.window
        if window is None:
            raise ValueError("pitch_wsola: a plan needs the window length (seal(..., window=W), or draw_one(W) before it)")
        plan = {"kind": "pitch_wsola", "n": len(entries), "window": int(window)}
        plan.update(pitch_tables(np.array(entries, dtype=np.int64).reshape(-1), window))
        plan["_dev"] = {k: _upload(plan[k], device) for k in ("cents", "ratio", "cutoff", "nominal")}
        return plan

    def apply(self, plan, lo, hi, src, dst=None, window=None):
        _check_src(src)
        window = _window(src, dst, window if window is not None else plan["window"])
        if window != plan["window"]:
            raise ValueError(f"pitch_wsola: the plan was sealed for windows of {plan['window']} samples, not {window}")
        b = hi - lo
        if not isinstance(src, FlatWindows) and dst is not None and src.data_ptr() == dst.data_ptr():
            src = src.clone()                                          # (out of place: every output reads many input samples)
        out = dst if dst is not None else torch.empty(b, window, dtype=torch.float32, device=_device_of(src))
        self.last_offsets = _pitch_launch(src, plan["_dev"], lo, hi, plan["cents_bound"], window, out)
        return out


# --------------------------------------------------------------------------- artificial reverberation
FREEVERB_COMB = (1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617)     # comb delays in samples at 44.1 kHz (the Freeverb network's)
FREEVERB_ALLPASS = (225, 341, 441, 556)                              # all-pass delays, likewise
FREEVERB_RHO = 16000 / 44100                                         # the effect is defined at 16 kHz only


def freeverb_tables(rooms, reverberance=100.0, hf_damping=100.0, wet_gain_dB=0.0):
    """The host tables of a batch of room sizes (FreeverbAugment's docstring), in f64: room [n] i32, comb_len [n, 8] i32 with
    D[c] = int(scale rho COMB[c] + 0.5) and scale = rs / 100 * 0.9 + 0.1, allpass_len (4 ints), feedback / damping / gain (each
    rounded once to f32, held as Python floats), feedback64 (the feedback before that rounding) and len_bound, the largest comb
    length (at least 1).  Refuses, by the argument's name, a room size outside [0, 100], reverberance or hf_damping outside
    [0, 100] and a wet_gain_dB that is not finite or whose gain does not fit float32."""
    rooms = np.asarray(rooms, dtype=np.int64).reshape(-1)
    if rooms.size and (int(rooms.min()) < 0 or int(rooms.max()) > 100):
        raise ValueError(f"a room size of {int(rooms.min() if rooms.min() < 0 else rooms.max())}: freeverb takes 0 to 100")
    if not 0 <= reverberance <= 100:
        raise ValueError(f"reverberance {reverberance}: freeverb takes 0 to 100")
    if not 0 <= hf_damping <= 100:
        raise ValueError(f"hf_damping {hf_damping}: freeverb takes 0 to 100")
    if not np.isfinite(wet_gain_dB):
        raise ValueError(f"wet_gain_dB {wet_gain_dB}: freeverb needs a finite gain")
    scale = rooms.astype(np.float64) / 100 * 0.9 + 0.1
    comb = (scale[:, None] * FREEVERB_RHO * np.array(FREEVERB_COMB, dtype=np.float64)[None, :] + 0.5).astype(np.int64)
    allpass = tuple(int(FREEVERB_RHO * a + 0.5) for a in FREEVERB_ALLPASS)
    a = -1 / np.log(0.7)
    b = 100 / (np.log(0.02) * a + 1)
    feedback = 1 - np.exp((reverberance - b) / (a * b))
    damping = hf_damping / 100 * 0.3 + 0.2
    gain = 0.015 * 10 ** (wet_gain_dB / 20)
    if not abs(gain) <= float(np.finfo(np.float32).max):
        raise ValueError(f"wet_gain_dB {wet_gain_dB}: the gain does not fit float32")
    return {"room": rooms.astype(np.int32), "comb_len": comb.astype(np.int32), "allpass_len": allpass,
            "feedback": float(np.float32(feedback)), "damping": float(np.float32(damping)), "gain": float(np.float32(gain)),
            "feedback64": float(feedback), "len_bound": max(int(comb.max()) if comb.size else 1, 1)}


def _freeverb_launch(src, comb_len, lo, hi, tables, window, out, what="augment_freeverb"):
    """cpc_augment_freeverb on rows [lo, hi) of the device table comb_len [n, 8] (int32)."""
    dev = _device_of(src)
    p, total, off = _operand(src)
    allpass = (ctypes.c_int * 4)(*tables["allpass_len"])
    check(_lib.load().cpc_augment_freeverb(p, total, off, ptr(comb_len[lo:hi]), int(tables["len_bound"]), allpass,
                                           tables["feedback"], tables["damping"], tables["gain"], ptr(out), hi - lo, window,
                                           stream_ptr(dev)), what)
    return out


class FreeverbAugment(_Transform):
    """`freeverb`: artificial reverberation of every window, with the room size drawn as the reference's ReverbAugment
    (data_augmentation.py: `random_room_size`) draws it -- ONE np.random.randint(0, room_max) per window from numpy's global
    generator, room_max = 100; the output has the input's length and is not peak-normalised.  The reference hands the number to
    sox's `reverb` effect -- reverb(reverberance = 100, hf_damping = 100, room); ReverbDropout uses (50, 50) -- which is not
    available.  The algorithm behind that effect is the public-domain Freeverb network, and what happens to the window here is
    THIS PACKAGE'S statement of it, written down below.  Its agreement with sox's output is unmeasured.  The constants are delays
    in samples at 44.1 kHz; the effect is defined at 16 kHz only.

      COMB = (1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617)    ALLPASS = (225, 341, 441, 556)    rho = 16000 / 44100

    Per window, on the host in f64 (`freeverb_tables`): rs the draw, scale = rs / 100 * 0.9 + 0.1,
      D[c] = int(scale * rho * COMB[c] + 0.5)        A[a] = int(rho * ALLPASS[a] + 0.5) = (82, 124, 160, 202)
      a = -1 / ln(0.7)    b = 100 / (ln(0.02) * a + 1)    fb = 1 - exp((reverberance - b) / (a * b))
      dmp = hf_damping / 100 * 0.3 + 0.2                g = 0.015 * 10 ** (wet_gain_dB / 20)
    and fb, dmp, g are rounded once to f32.  The defaults (100, 100, 0 dB) give fb = 0.98 and dmp = 0.5; (50, 50) gives
    fb = 0.8816784043380077 and dmp = 0.35.  rs = 0 gives D = (40, 43, 46, 49, 52, 54, 56, 59), rs = 99 gives
    D = (401, 427, 459, 488, 511, 536, 560, 581).

    The window x[0 .. W) is f32; all state is zero at n = 0 and nothing outside the window is read, whatever lies beside it in a
    pack.  For n = 0 .. W - 1, in f32:

      u = g * x[n];  acc = 0
      for c in 0..7:   o = line_c[p_c];  s_c = o + (s_c - o) * dmp;  line_c[p_c] = u + s_c * fb;  p_c = (p_c + 1) % D[c];  acc = acc + o
      v = acc
      for a in 0..3:   o = line_a[p_a];  line_a[p_a] = v + o * 0.5;  v = o - v;  p_a = (p_a + 1) % A[a]
      y[n] = x[n] + v

    No pre-delay, no tone filters, no stereo spread (one mono bank), no dither, no clipping, no peak normalisation; the tail beyond
    W is cut off, as natural_reverb cuts it.  On the device (csrc/freeverb.hip) one workgroup per window keeps the twelve lines in
    LDS and performs exactly these operations in this order, so a window's bits depend on nothing else in the batch or the pack.

    Entry: rs.  Plan: room [n] i32, comb_len [n, 8] i32, allpass_len, feedback, damping, gain, len_bound.  Out of place."""

    def __init__(self, room_max=100, reverberance=100.0, hf_damping=100.0, wet_gain_dB=0.0):
        if not np.isfinite(room_max) or room_max != int(room_max):
            raise ValueError(f"room_max {room_max}: freeverb draws a whole room size from [0, room_max)")
        if not 1 <= room_max <= 100:
            raise ValueError(f"room_max {room_max}: freeverb draws the room size from [0, room_max), room_max from 1 to 100")
        freeverb_tables([], reverberance, hf_damping, wet_gain_dB)      # (refuses the other three by name, a gain beyond float32 too)
        self.room_max = int(room_max)
        self.reverberance = float(reverberance)
        self.hf_damping = float(hf_damping)
        self.wet_gain_dB = float(wet_gain_dB)

    def draw_one(self, window):
        return int(np.random.randint(0, self.room_max))

    def seal(self, entries, device):
        plan = {"kind": "freeverb", "n": len(entries)}
        plan.update(freeverb_tables(np.array(entries, dtype=np.int64).reshape(-1), self.reverberance, self.hf_damping,
                                    self.wet_gain_dB))
        plan["_dev"] = {"comb_len": _upload(plan["comb_len"], device)}
        return plan

    def apply(self, plan, lo, hi, src, dst=None, window=None):
        _check_src(src)
        window = _window(src, dst, window)
        if not isinstance(src, FlatWindows) and dst is not None and src.data_ptr() == dst.data_ptr():
            src = src.clone()                                          # (out of place: the kernel refuses out == src)
        out = dst if dst is not None else torch.empty(hi - lo, window, dtype=torch.float32, device=_device_of(src))
        _freeverb_launch(src, plan["_dev"]["comb_len"], lo, hi, plan, window, out)
        return out


# --------------------------------------------------------------------------- band reject
BANDREJECT_SR = 16000                                                # the transform is defined at 16 kHz only
BANDREJECT_MEL_STEPS, BANDREJECT_WIDTH = 256, 27                     # the reference's n_mels and F (data_augmentation.py:40-49)
BANDREJECT_MAX_HALF = 1024                                           # cpc_bandreject_max_half()


def bandreject_tables(low, high, attenuation_dB=120.0, transition_hz=400.0, sr=BANDREJECT_SR):
    """The host tables of a batch of bands (BandrejectSincAugment's docstring), in f64: band [n, 2] (low, high in Hz), beta, half
    (H) and taps (2 H + 1).  Refuses, by the argument's name, a band that is not finite or outside 0 <= low <= high <= sr / 2, an
    attenuation outside (50, 140] and a transition width whose half length falls outside [1, 1024]."""
    low = np.asarray(low, dtype=np.float64).reshape(-1)
    high = np.asarray(high, dtype=np.float64).reshape(-1)
    if not np.isfinite(sr) or sr <= 0:
        raise ValueError(f"sr {sr}: bandreject_sinc needs a positive sample rate")
    if not np.isfinite(low).all() or (low < 0).any():
        raise ValueError(f"low {low[~(np.isfinite(low) & (low >= 0))][0]}: bandreject_sinc takes a band 0 <= low <= high <= sr / 2")
    if not np.isfinite(high).all() or (high > sr / 2).any():
        raise ValueError(f"high {high[~(np.isfinite(high) & (high <= sr / 2))][0]}: bandreject_sinc takes a band "
                         f"0 <= low <= high <= sr / 2 = {sr / 2}")
    if low.size != high.size:
        raise ValueError(f"high: {high.size} upper edges for {low.size} lower edges")
    if (low > high).any():
        raise ValueError(f"low {low[low > high][0]} above high {high[low > high][0]}: bandreject_sinc takes a band "
                         "0 <= low <= high <= sr / 2")
    if not 50 < attenuation_dB <= 140:
        raise ValueError(f"attenuation_dB {attenuation_dB}: bandreject_sinc takes more than 50 and at most 140 dB")
    if not transition_hz > 0 or not np.isfinite(transition_hz):
        raise ValueError(f"transition_hz {transition_hz}: bandreject_sinc needs a positive finite transition width")
    beta = 0.1102 * (attenuation_dB - 8.7)
    dw = 2 * np.pi * transition_hz / sr
    order = np.ceil((attenuation_dB - 7.95) / (2.285 * dw))
    if not order < 2 ** 31:
        raise ValueError(f"transition_hz {transition_hz}: a filter of {order:.3g} taps; at most {2 * BANDREJECT_MAX_HALF + 1} are built")
    half = (int(order) + 1) // 2
    if not 1 <= half <= BANDREJECT_MAX_HALF:
        raise ValueError(f"transition_hz {transition_hz}: {attenuation_dB} dB over {transition_hz} Hz at {sr} Hz needs a half length of "
                         f"{half} taps; 1 to {BANDREJECT_MAX_HALF} are built")
    return {"band": np.stack([low, high], axis=1), "half": half, "beta": float(beta), "taps": 2 * half + 1}


def _bandreject_launch(src, band, lo, hi, tables, window, out, what="augment_bandreject"):
    """cpc_augment_bandreject on rows [lo, hi) of the device table band [n, 2] (float64)."""
    dev = _device_of(src)
    p, total, off = _operand(src)
    check(_lib.load().cpc_augment_bandreject(p, total, off, ptr(band[lo:hi]), int(tables["half"]), float(tables["beta"]),
                                             float(BANDREJECT_SR), ptr(out), hi - lo, window, stream_ptr(dev)), what)
    return out


class BandrejectSincAugment(_Transform):
    """`bandreject_sinc`: one frequency band of every window rejected, with the band drawn as the reference's BandrejectAugment
    (data_augmentation.py:40-49, `generate_freq_mask`) draws it -- TWO np.random.uniform calls per window from numpy's global
    generator, on the mel scale; the output has the input's length and is not peak-normalised.  The reference hands the band to a
    sox effect chain (`sinc -a 120 high-low`, then `dither`) that is not available.  The textbook filter behind that chain is a
    Kaiser-windowed sinc band-reject FIR, and what happens to the window here is THIS PACKAGE'S statement of one, written down
    below.  Its agreement with sox's output is unmeasured, and there is no dither.  The transform is defined at sr = 16000 only.

    The draw, per window and in this order:
      F = 27 scaler    melfmax = 2595 log10(1 + 8000 / 700)
      meldf = uniform(0, melfmax F / 256)    melf0 = uniform(0, melfmax - meldf)
      low = mel2freq(melf0)    high = mel2freq(melf0 + meldf)    mel2freq(m) = (10 ** (m / 2595) - 1) 700
    `scaler` (--bandreject_scaler) must be finite with 0 <= 27 scaler <= 256, or the draw would leave [0, 8000].

    The filter, from the attenuation A in dB (120) and the transition width tbw in Hz (400, 5 % of the 8 kHz band), on the host
    in f64 (`bandreject_tables`):
      beta = 0.1102 (A - 8.7)    dw = 2 pi tbw / sr    M = ceil((A - 7.95) / (2.285 dw))    H = (M + 1) // 2    T = 2 H + 1 taps
    The defaults give beta = 12.26526, M = 313, H = 157, T = 315.  For j = -H .. H:
      w[j]    = I0(beta sqrt(1 - (j / H) ** 2)) / I0(beta)
      lp_f[j] = (2 f / sr) sinc(2 f j / sr)        sinc(u) = sin(pi u) / (pi u), sinc(0) = 1
      h[j]    = [j == 0] - w[j] (lp_high[j] - lp_low[j])                  (no renormalisation)
      y[t]    = round_f32( sum_{j = -H .. H} h[j] x[t - j] ),  t = 0 .. W - 1
    Every product and sum is in f64 in one fixed order; x is f32 and reads as zero outside the window's own [0, W), whatever lies
    beside it in a pack.  No dither, no clipping, no peak normalisation.  A window with low == high is the identity and is COPIED
    with no arithmetic; so is a window whose pair is no band (the table lives on the device and is not read back).

    On the device (csrc/bandreject.hip) every workgroup designs its window's H + 1 taps in f64 -- I0 from its power series, the
    sine from an argument reduced exactly, each tap within 2 ** -40 of its value -- and sums h[0] x[t], then
    fma(h[j], x[t - j] + x[t + j], .) for j = 1 .. H, rounding once at the store, so a window's bits depend on nothing else in the
    batch or the pack and a plan costs two doubles per window.

    Entry: (low, high).  Plan: low [n] f64, high [n] f64, band [n, 2] f64, half, beta, taps.  Out of place."""

    def __init__(self, scaler=1.0, attenuation_dB=120.0, transition_hz=400.0):
        if not np.isfinite(scaler) or not 0 <= BANDREJECT_WIDTH * scaler <= BANDREJECT_MEL_STEPS:
            raise ValueError(f"scaler {scaler}: bandreject_sinc draws a band of at most 27 scaler of 256 mel steps, scaler from 0 to "
                             f"{BANDREJECT_MEL_STEPS / BANDREJECT_WIDTH:.4f}")
        bandreject_tables([], [], attenuation_dB, transition_hz)        # (refuses the other two by name)
        self.scaler = float(scaler)
        self.attenuation_dB = float(attenuation_dB)
        self.transition_hz = float(transition_hz)

    @staticmethod
    def mel2freq(mel):
        return (10 ** (mel / 2595) - 1) * 700

    def draw_one(self, window):
        width = BANDREJECT_WIDTH * self.scaler
        melfmax = 2595 * np.log10(1 + (BANDREJECT_SR / 2) / 700)
        meldf = np.random.uniform(0, melfmax * width / BANDREJECT_MEL_STEPS)
        melf0 = np.random.uniform(0, melfmax - meldf)
        return float(self.mel2freq(melf0)), float(self.mel2freq(melf0 + meldf))

    def seal(self, entries, device):
        arr = np.array(entries, dtype=np.float64).reshape(-1, 2)
        plan = {"kind": "bandreject_sinc", "n": len(arr)}
        high = np.minimum(arr[:, 1], BANDREJECT_SR / 2)                # (a draw at the very top of the scale may round a hair past 8000 Hz)
        plan.update(bandreject_tables(arr[:, 0], high, self.attenuation_dB, self.transition_hz))
        plan["low"], plan["high"] = plan["band"][:, 0].copy(), plan["band"][:, 1].copy()
        plan["_dev"] = {"band": _upload(plan["band"], device)}
        return plan

    def apply(self, plan, lo, hi, src, dst=None, window=None):
        _check_src(src)
        window = _window(src, dst, window)
        if not isinstance(src, FlatWindows) and dst is not None and src.data_ptr() == dst.data_ptr():
            src = src.clone()                                          # (out of place: every output reads many input samples)
        out = dst if dst is not None else torch.empty(hi - lo, window, dtype=torch.float32, device=_device_of(src))
        _bandreject_launch(src, plan["_dev"]["band"], lo, hi, plan, window, out)
        return out


# --------------------------------------------------------------------------- combinations
class CombinedTransforms(_Transform):
    """data_augmentation.py:331-344: the transforms of `augment_cfgs`, applied in the order given ('none' entries skipped).
    Entry: the tuple of the parts' entries (drawn in that order, window by window).  Plan: {"parts": [plan, ...]}."""

    def __init__(self, augment_cfgs, **kwargs):
        self.transfors_cfgs = [get_augment(x, **kwargs) for x in augment_cfgs]
        self._parts = [t for t in self.transfors_cfgs if t is not None]
        self._draws = [t.draw_one for t in self._parts]

    def draw_one(self, window):
        return tuple([draw(window) for draw in self._draws])

    def seal(self, entries, device):
        parts = self._parts
        return {"kind": "combined", "n": len(entries),
                "parts": [t.seal([e[i] for e in entries], device) for i, t in enumerate(parts)]}

    def apply(self, plan, lo, hi, src, dst=None, window=None):
        parts = self._parts
        out_of_place = [i for i, t in enumerate(parts) if not t.inplace]
        last = out_of_place[-1] if out_of_place else -1
        window = _window(src, dst, window)
        cur = src
        for i, (t, p) in enumerate(zip(parts, plan["parts"])):
            target = dst if i >= last else None            # from the last out-of-place stage on, everything happens in dst
            cur = t.apply(p, lo, hi, cur, target, window=window)
        if dst is not None and cur is not dst:             # (no stage at all, or in-place stages on a caller's buffer)
            cur = _buffer(cur, window, dst) if isinstance(cur, FlatWindows) else dst.copy_(cur.view_as(dst))
        return cur

    def __call__(self, x):
        _lib.require_gpu(x)
        rows = _rows(x.contiguous())
        plan = self.plan(rows.size(0), x.shape[-1], x.device)
        self.last_plan = plan
        return _rows(self.apply(plan, 0, rows.size(0), rows.clone())).view(x.shape)


def get_augment(augment_type, **kwargs):
    """data_augmentation.py:347-378."""
    if not augment_type or augment_type == 'none':
        return None
    if augment_type == 'additive':
        if not kwargs['noise_dataset']:
            raise RuntimeError('Noise dataset is needed for the additive noise')
        return AdditiveNoiseAugment(kwargs['noise_dataset'], kwargs['additive_noise_snr_min'],
                                    kwargs['additive_noise_snr_max'], kwargs['batchSize'], kwargs['additive_noise_sampling'])
    if augment_type == 'time_dropout':
        return TimeDropoutAugment(kwargs['t_ms'])
    if augment_type == 'natural_reverb':
        return NaturalReverb(ir_paths=kwargs['pathImpulseResponses'], p=kwargs['impulse_response_prob'],
                             batchSize=kwargs['batchSize'], sr=kwargs['ir_sample_rate'], batch_wise=kwargs['ir_batch_wise'])
    if augment_type == 'pitch_wsola':
        return PitchShiftAugment(kwargs['shift_max'])
    if augment_type == 'freeverb':
        return FreeverbAugment()
    if augment_type == 'bandreject_sinc':
        return BandrejectSincAugment(kwargs.get('bandreject_scaler', 1.0))
    if augment_type in UNBUILT_TYPES:
        raise NotImplementedError(unbuilt_message(augment_type))
    raise RuntimeError(f'Unknown augment_type = {augment_type}')


def augmentation_factory(args, noise_dataset=None, applied_on_noise=False):
    """data_augmentation.py:381-442: None when no half is augmented or the type is none; one type gives its class, several give
    CombinedTransforms; `applied_on_noise` reads --meta_aug_type / --meta_ir_batch_wise instead (the reverberated noise).  A
    request that names an unbuilt type raises NotImplementedError before anything is built."""
    if applied_on_noise:
        augment_type = args.meta_aug_type
        ir_batch_wise = args.meta_ir_batch_wise
        if augment_type is not None:
            print("Activating meta data augmentation with : %s" % augment_type)
    else:
        augment_type = args.augment_type
        ir_batch_wise = args.ir_batch_wise
        print("Activating data augmentation with : %s" % augment_type)

    if not augment_type or augment_type == 'none' or list(augment_type) == ['none'] or \
            not (args.augment_past or args.augment_future):
        return None
    if isinstance(augment_type, str):
        augment_type = [augment_type]
    if any(t in UNBUILT_TYPES for t in augment_type):
        raise NotImplementedError(unbuilt_message(augment_type))

    batchSize = args.nGPU * args.batchSizeGPU
    additive_noise_sampling = "temporalsamespeaker" if args.temporal_additive_noise else "uniform"
    aug_args = {"t_ms": args.t_ms,
                "bandreject_scaler": args.bandreject_scaler,
                "shift_max": args.shift_max,
                "noise_dataset": noise_dataset,
                "additive_noise_snr_min": args.min_snr_in_db,
                "additive_noise_snr_max": args.max_snr_in_db,
                "additive_noise_sampling": additive_noise_sampling,
                "impulse_response_prob": args.impulse_response_prob,
                "pathImpulseResponses": args.pathImpulseResponses,
                "ir_sample_rate": args.ir_sample_rate,
                "batchSize": batchSize,
                "ir_batch_wise": ir_batch_wise}
    if len(augment_type) > 1:
        return CombinedTransforms(augment_type, **aug_args)
    return get_augment(augment_type[0], **aug_args)
