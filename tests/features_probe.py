"""A probe feature maker for feature_loader's readers (tools/make_golden_features.py, tests/test_features_cpu.py): its output says,
frame by frame, which sample of the file the frame starts at, how long the call it came from was and how many rows that call had.
With the waveform arange(n) (exact in f32 below 2^24) the result of buildFeature / buildFeature_batch is then a record of the
plan the reader followed -- chunks, rest, strict tail, batching -- in integers."""
import numpy as np
import torch

GEOMETRY = ((10, 5, 3), (8, 4, 2), (4, 2, 1), (4, 2, 1), (4, 2, 1))      # (kernel, stride, padding) of the encoder's convolutions


def frames(length):
    """Output frames of the five convolutions on `length` samples (cpc_encoder_frames)."""
    for k, s, p in GEOMETRY:
        length = (length + 2 * p - k) // s + 1
    return length


class ProbeMaker(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.dummy = torch.nn.Parameter(torch.zeros(1))

    def getDownsamplingFactor(self):
        return 160

    def forward(self, data):
        x, _ = data
        rows, _, length = x.shape
        n = frames(length)
        if n < 1:
            raise ValueError(f"{length} samples leave no frame")
        out = torch.empty(rows, n, 3, dtype=torch.float32)
        out[:, :, 0] = x[:, 0, 0:160 * n:160]
        out[:, :, 1] = length
        out[:, :, 2] = rows
        return out


def encode(out):
    """[1, frames, 3] probe features -> int64 [runs, 4]: (first sample, frames, call length, call rows) of every maximal run of
    frames 160 samples apart that share a call length and row count.  Lossless: equal codes <=> equal outputs."""
    a = out.reshape(-1, 3).double().numpy()
    assert np.all(a == np.round(a))
    a = a.astype(np.int64)
    runs = []
    for sample, length, rows in a:
        if runs and runs[-1][2] == length and runs[-1][3] == rows and runs[-1][0] + 160 * runs[-1][1] == sample:
            runs[-1][1] += 1
        else:
            runs.append([sample, 1, length, rows])
    return np.asarray(runs, dtype=np.int64).reshape(-1, 4)


def sweep_cases():
    """(reader, maxSizeSeq, strict, batch_size or 0, n) of the provenance sweep."""
    out = []
    for C in (8000, 10000, 64000):
        ns = [159, 160, 400, C // 2, C - 1, C, C + 1, C + 158, C + 159, C + 160, C + 161, C + 399, C + 400, 2 * C - 1, 2 * C,
              3 * C + 6900]
        for strict in (False, True):
            for n in ns:
                out.append(("buildFeature", C, strict, 0, n))
                for bs in (1, 3, 8):
                    out.append(("buildFeature_batch", C, strict, bs, n))
    return out


def sweep_key(case):
    reader, C, strict, bs, n = case
    return f"prov/{reader}/C{C}/{'strict' if strict else 'loose'}/b{bs}/n{n}"


def wide_params(cfg):
    """The state dict (oracle/synth parameters) of a hidden 256 / 512 model of g25_features.json's "models"."""
    from oracle import synth
    h = cfg["hidden"]
    p = synth.encoder_params(h, cfg["enc_seed"])
    if cfg["ar"] == "transformer":
        p.update(synth.transformer_params(h, h, cfg["size_seq"], cfg["ar_seed"], prefix="gAR.0."))
    elif cfg["ar"] == "LSTM":
        p.update(synth.lstm_params(h, h, cfg["layers"], cfg["ar_seed"]))
    else:
        p.update(synth.gru_params(h, h, cfg["layers"], cfg["ar_seed"]))
    return p
