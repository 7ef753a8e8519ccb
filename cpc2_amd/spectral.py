"""Log-mel filterbanks and MFCCs on the device without torchaudio (absent from the image): the baseline features every CPC /
ZeroSpeech table prints beside a model's score (csrc/mfcc.hip; the C ABI and the definition are in include/cpc2_hip.h, the
argument in DESIGN.md section 18; `python -m cpc2_amd.eval.build_baseline_features` writes them to files).

The definition restates torchaudio's documented Spectrogram / MelScale / AmplitudeToDB / create_dct / compute_deltas.  IT HAS
NEVER BEEN COMPARED WITH A TORCHAUDIO BINARY: agreement with torchaudio itself is unmeasured.  For a signal x[0 .. L):

  frames   frame t is centred on c_t = t * hop + offset and reads xr[c_t - n_fft // 2 + n], n < n_fft; xr is x reflected without
           repeating the edge sample (i < 0 -> -i, i >= L -> 2 (L - 1) - i), so L <= n_fft // 2 is refused.
           grid="center": offset 0, 1 + L // hop frames (torchaudio's center=True, the reference's MFCCEncoder);
           grid="cpc":    offset hop // 2, L // hop frames: frame t sits on the centre of CPC frame t, the grid ABXFeatureLoader
                          and the phone labels assume.
  window   periodic Hann of n_fft points;  power  |DFT|^2 for k <= n_fft // 2, no normalisation
  mel      HTK scale, norm=None, all_freqs = linspace(0, sample_rate // 2, n_freqs); all-zero filters stay zero
  dB       10 log10(max(., 1e-10)), then max(., max - top_db): the outer max over one signal (floor="signal": a file's features do
           not depend on what it was batched with) or over the whole call (floor="call": torchaudio on a 3-D batch)
  mfcc     the first n_mfcc rows of the orthonormal DCT-II over the mel axis
  deltas   d[t] = sum_{j=1,2} j (c[t+j] - c[t-j]) / 10 with replicate edges, from the stored f32 values; order 2 is the delta of
           the stored order 1; each order is appended along the feature axis

Everything between the f32 samples and the f32 store is f64 (tables built on the host in double, sums on the f64 matrix
instruction, f64 log10), and there is no float atomic: the same call gives the same bits, and with floor="signal" a signal in a
pack gives the bits it gives alone."""
import torch

from . import _lib

FRAME_TILE = 16                     # frames per workgroup (cpc_mfcc_frame_tile(); tests/test_mfcc_cpu.py holds the two together)
MIN_N_FFT, MAX_N_FFT, MAX_N_MELS = 32, 512, 512
MAX_DELTA_SIGNALS = 65535           # signals per launch of the deltas kernel
GRIDS = ("cpc", "center")
FLOORS = ("signal", "call")


def check_parameters(n_fft, hop, n_mels, n_out, top_db=None, grid="cpc", floor="signal", sample_rate=16000, f_min=0.0, f_max=None):
    """The kernel's domain, each refusal naming its parameter (ValueError); nothing is launched or read."""
    if not MIN_N_FFT <= int(n_fft) <= MAX_N_FFT:
        raise ValueError(f"n_fft={n_fft} is outside the kernel's domain {MIN_N_FFT}..{MAX_N_FFT}")
    if not 1 <= int(hop) <= int(n_fft):
        raise ValueError(f"hop={hop} is outside 1..n_fft (n_fft={n_fft})")
    if not 1 <= int(n_mels) <= MAX_N_MELS:
        raise ValueError(f"n_mels={n_mels} is outside the kernel's domain 1..{MAX_N_MELS}")
    if not 1 <= int(n_out) <= int(n_mels):
        raise ValueError(f"n_mfcc={n_out} is outside 1..n_mels (n_mels={n_mels})")
    if top_db is not None and not (0.0 <= float(top_db) < float("inf")):
        raise ValueError(f"top_db={top_db}: a finite value >= 0, or None")
    if grid not in GRIDS:
        raise ValueError(f"grid={grid!r}: one of {GRIDS}")
    if floor not in FLOORS:
        raise ValueError(f"floor={floor!r}: one of {FLOORS}")
    if int(sample_rate) < 2:
        raise ValueError(f"sample_rate={sample_rate}")
    top = float(int(sample_rate) // 2) if f_max is None else float(f_max)
    if not 0.0 <= float(f_min) < top:
        raise ValueError(f"need 0 <= f_min < f_max (f_min={f_min}, f_max={top})")


def host_tables(n_fft, n_mels, n_out, sample_rate=16000, f_min=0.0, f_max=None):
    """The kernels' one table buffer (float64, host): window | cos | sin | filterbank | dct^T, as cpc2_hip.h lays it out."""
    lib = _lib.load()
    count = lib.cpc_mfcc_tables_doubles(int(n_fft), int(n_mels), int(n_out))
    if count <= 0:
        raise ValueError(lib.cpc_last_error().decode(errors="replace"))
    tables = torch.empty(count, dtype=torch.float64)
    top = float(int(sample_rate) // 2) if f_max is None else float(f_max)
    _lib.check(lib.cpc_mfcc_tables_host(int(n_fft), int(n_mels), int(n_out), int(sample_rate), float(f_min), top,
                                        _lib.ptr(tables), count), "mfcc_tables_host")
    return tables


def _exclusive(values):
    out, total = [], 0
    for v in values:
        out.append(total)
        total += v
    return out, total


def _deltas_launch(buf, src_col, dst_col, cols, frames, rows):
    """buf[:, dst_col : dst_col + cols] = deltas of buf[:, src_col : src_col + cols], signal i on rows rows[i] .. + frames[i]."""
    lib, device = _lib.load(), buf.device
    for a in range(0, len(frames), MAX_DELTA_SIGNALS):
        fr, ro = frames[a:a + MAX_DELTA_SIGNALS], rows[a:a + MAX_DELTA_SIGNALS]
        if max(fr) < 1:
            continue
        tables = torch.tensor([fr, ro], dtype=torch.int64).to(device)
        _lib.check(lib.cpc_deltas(buf.data_ptr() + 4 * src_col, buf.stride(0), buf.data_ptr() + 4 * dst_col, buf.stride(0), cols,
                                  _lib.ptr(tables[0]), _lib.ptr(tables[1]), len(fr), max(fr), buf.size(0),
                                  _lib.stream_ptr(device)), "deltas")


def compute_deltas(features, lengths=None, order=1):
    """features [rows, D] (signal i on the next lengths[i] rows; one signal when lengths is None) or a batch [b, T, D], float32
    on the device.  Returns the features with `order` (0, 1 or 2) delta blocks appended along the last axis."""
    _lib.require_gpu(features)
    if order not in (0, 1, 2):
        raise ValueError(f"deltas of order {order}: 0, 1 or 2")
    x = _lib.f32c(features)
    if x.dim() == 3:
        if lengths is not None:
            raise ValueError("compute_deltas: a [b, T, D] batch has T frames per signal; lengths belong to packed rows")
        frames = [x.size(1)] * x.size(0)
    elif x.dim() == 2:
        frames = [x.size(0)] if lengths is None else [int(v) for v in lengths]
        if any(v < 0 for v in frames) or sum(frames) > x.size(0):
            raise ValueError("compute_deltas: the lengths leave the rows")
    else:
        raise ValueError(f"compute_deltas takes [rows, D] or [b, T, D], got {tuple(x.shape)}")
    d = x.size(-1)
    flat = x.reshape(-1, d)
    out = torch.empty(flat.size(0), d * (1 + order), dtype=torch.float32, device=x.device)
    out[:, :d] = flat
    if order and flat.size(0) and d and frames:
        rows, _ = _exclusive(frames)
        for o in range(order):
            _deltas_launch(out, o * d, (o + 1) * d, d, frames, rows)
    return out.view(x.shape[:-1] + (d * (1 + order),))


class MelSpectrogramDB:
    """Log-mel filterbank energies in dB: `obj(batch)` for a [b, L] / [b, 1, L] device batch gives [b, T, n_mels * (1 + deltas)];
    `obj(signals)` for a list of 1-D device tensors, or `obj(flat, lengths=..., offsets=...)` for a pack as
    audio.resample_pack takes it, gives a list of [T_i, .] views of ONE output matrix (signal i on rows row_offsets[i] ..;
    `out` / `row_offsets` place it in a matrix of the caller's, of which nothing else is written)."""
    kind = "mel"

    def __init__(self, sample_rate=16000, n_fft=400, hop=160, n_mels=40, f_min=0.0, f_max=None, top_db=80.0, floor="signal",
                 grid="cpc"):
        self.sample_rate, self.n_fft, self.hop, self.n_mels = int(sample_rate), int(n_fft), int(hop), int(n_mels)
        self.f_min, self.f_max = float(f_min), None if f_max is None else float(f_max)
        self.top_db = None if top_db is None else float(top_db)
        self.floor, self.grid = floor, grid
        self.n_out = self._n_out()
        check_parameters(self.n_fft, self.hop, self.n_mels, self.n_out, self.top_db, grid, floor, self.sample_rate, self.f_min,
                         self.f_max)
        self.offset = self.hop // 2 if grid == "cpc" else 0
        self._tables = {}

    def _n_out(self):
        return self.n_mels

    def n_frames(self, length):
        return int(length) // self.hop if self.grid == "cpc" else 1 + int(length) // self.hop

    def tables(self, device):
        """The table buffer on `device`: built on the host in double once, uploaded once per device."""
        key = (device.type, _lib.device_index(device))
        if key not in self._tables:
            if "host" not in self._tables:
                self._tables["host"] = host_tables(self.n_fft, self.n_mels, self.n_out, self.sample_rate, self.f_min, self.f_max)
            self._tables[key] = self._tables["host"].to(device)
        return self._tables[key]

    def __call__(self, signals, lengths=None, offsets=None, deltas=0, out=None, row_offsets=None):
        if deltas not in (0, 1, 2):
            raise ValueError(f"deltas of order {deltas}: 0, 1 or 2")
        if isinstance(signals, (list, tuple)):
            if not signals:
                return []
            _lib.require_gpu(*signals)
            if any(s.dim() != 1 for s in signals):
                raise ValueError("a list holds 1-D signals (or pass a flat vector with lengths)")
            lengths = [int(s.numel()) for s in signals]
            return self._pack(torch.cat([_lib.f32c(s) for s in signals]), lengths, None, deltas, out, row_offsets)
        _lib.require_gpu(signals)
        if lengths is not None:
            return self._pack(_lib.f32c(signals).view(-1), [int(v) for v in lengths], offsets, deltas, out, row_offsets)
        x = _lib.f32c(signals)
        if x.dim() == 3 and x.size(1) == 1:
            x = x[:, 0]
        if x.dim() != 2:
            raise ValueError(f"a batch is [b, L] or [b, 1, L] (got {tuple(signals.shape)}); a pack needs lengths")
        b, length = x.shape
        if b == 0:
            return torch.empty(0, self.n_frames(length), self.n_out * (1 + deltas), dtype=torch.float32, device=x.device)
        rows = self._pack(x.reshape(-1), [length] * b, None, deltas, out, row_offsets)
        return torch.stack(rows)

    def _pack(self, flat, lengths, offsets, deltas, out, row_offsets):
        lib, device = _lib.load(), flat.device
        count = len(lengths)
        if offsets is None:
            offsets, _ = _exclusive(lengths)
        offsets = [int(v) for v in offsets]
        if len(offsets) != count or any(a < 0 or a + b > flat.numel() for a, b in zip(offsets, lengths)):
            raise ValueError("a signal leaves the flat vector")
        short = [v for v in lengths if v <= self.n_fft // 2]
        if short:
            raise ValueError(f"a signal of {short[0]} samples is too short: reflection needs more than n_fft // 2 = "
                             f"{self.n_fft // 2} samples")
        frames = [self.n_frames(v) for v in lengths]
        width = self.n_out * (1 + deltas)
        if row_offsets is None:
            row_offsets, _ = _exclusive(frames)
        row_offsets = [int(v) for v in row_offsets]
        if out is None:
            out = torch.empty(max([a + b for a, b in zip(row_offsets, frames)] + [0]), width, dtype=torch.float32, device=device)
        else:
            _lib.require_gpu(out)
            if out.dtype != torch.float32 or out.dim() != 2 or out.stride(1) != 1 or out.size(1) < width or out.device != device:
                raise TypeError(f"out is a float32 matrix [rows, >= {width}] with unit column stride on the signals' device")
        if len(row_offsets) != count or any(a < 0 or a + b > out.size(0) for a, b in zip(row_offsets, frames)):
            raise ValueError("a result leaves the output matrix")
        tiles = [(v + FRAME_TILE - 1) // FRAME_TILE for v in frames]
        tile_start, total_tiles = _exclusive(tiles)
        if total_tiles:
            meta = torch.tensor([offsets + [0], lengths + [0], frames + [0], row_offsets + [0], tile_start + [total_tiles]],
                                dtype=torch.int64).to(device)
            tables = self.tables(device)
            nbytes = lib.cpc_melspec_scratch_bytes(total_tiles, count, self.n_mels)
            if nbytes == 0:
                raise ValueError(lib.cpc_last_error().decode(errors="replace"))
            scratch = _lib.scratch(nbytes, device)
            floor_mode = 0 if self.top_db is None else 1 + FLOORS.index(self.floor)
            stream = _lib.stream_ptr(device)
            _lib.check(lib.cpc_melspec_db(_lib.ptr(flat), flat.numel(), _lib.ptr(meta[0]), _lib.ptr(meta[1]), _lib.ptr(meta[2]),
                                          _lib.ptr(meta[4]), count, total_tiles, min(lengths), self.n_fft, self.hop, self.offset,
                                          self.n_mels, _lib.ptr(tables), floor_mode, 0.0 if self.top_db is None else self.top_db,
                                          _lib.ptr(scratch), scratch.numel(), stream), "melspec_db")
            _lib.check(lib.cpc_mfcc_finish(_lib.ptr(scratch), scratch.numel(), _lib.ptr(meta[2]), _lib.ptr(meta[3]), _lib.ptr(meta[4]),
                                           count, total_tiles, self.n_fft, self.n_mels, self.n_out, int(self.kind == "mfcc"),
                                           _lib.ptr(tables), floor_mode, _lib.ptr(out), out.stride(0), out.size(0), stream),
                       "mfcc_finish")
            for o in range(deltas):
                _deltas_launch(out, o * self.n_out, (o + 1) * self.n_out, self.n_out, frames, row_offsets)
        return [out[a:a + b, :width] for a, b in zip(row_offsets, frames)]


class MFCC(MelSpectrogramDB):
    """The first n_mfcc DCT-II coefficients (norm="ortho") of MelSpectrogramDB's rows; called the same way."""
    kind = "mfcc"

    def __init__(self, sample_rate=16000, n_mfcc=13, n_fft=400, hop=160, n_mels=40, f_min=0.0, f_max=None, top_db=80.0,
                 floor="signal", grid="cpc"):
        self.n_mfcc = int(n_mfcc)
        super().__init__(sample_rate, n_fft, hop, n_mels, f_min, f_max, top_db, floor, grid)

    def _n_out(self):
        return self.n_mfcc

    @classmethod
    def reference_encoder(cls, dimEncoded):
        """The configuration of the reference's MFCCEncoder (cpc/model.py:111-125: torchaudio.transforms.MFCC(n_mfcc=dimEncoded,
        melkwargs={"n_mels": max(128, dimEncoded), "n_fft": 321}) on a batch): hop 160, centred frames, top_db 80 over the call."""
        return cls(sample_rate=16000, n_mfcc=int(dimEncoded), n_fft=321, hop=160, n_mels=max(128, int(dimEncoded)), top_db=80.0,
                   floor="call", grid="center")
