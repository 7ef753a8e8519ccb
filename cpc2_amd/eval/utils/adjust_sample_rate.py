"""Bring the audio files of a directory to one sample rate (the reference's cpc/eval/utils/adjust_sample_rate.py): the window
feeder takes a file's samples as they come, whatever its rate, so a corpus is converted to 16 kHz before training or evaluation,
and impulse responses to --ir_sample_rate before natural_reverb reads them.

    python -m cpc2_amd.eval.utils.adjust_sample_rate path_db [path_phone_files] path_out [--out_sample_rate 16000]
                                                     [--file_extension .wav] [--recursive]

The reference's arguments and function names (adjust_sample_rate, get_names_list, parse_args, main) and its file selection: the
flat listing of path_db, files with the given suffix whose stem is in the first column of the phone file, both lists sorted and
merged.  The conversion is torchaudio's sinc_interp_hann resampler (the reference's torchaudio.transforms.Resample) as one kernel
launch per pack of files (cpc2_amd.audio.resample_pack), quantised to 16 bits on the device.

Deviations from the reference:
  * --file_extension defaults to .wav (the reference: .mp3).  There is no mp3 decoder here: .mp3 is refused by name before
    anything is read, and only .wav and .flac are accepted.
  * path_phone_files may be left out (two positional arguments: path_db path_out): every file with the suffix is converted.
    Noise and impulse-response directories have no transcriptions.
  * --recursive walks the sub-directories of path_db and mirrors them under path_out (the phone file still selects by stem).
  * The output is always 16-bit PCM .wav under the input's stem (the reference keeps the input's name and lets the container
    follow it).  Samples beyond [-1, 1) are clamped; one line reports how many were.
  * A path_out that exists and is not empty is refused: nothing is overwritten.
  * The reference's merge reads past the end of the phone list when the directory has names beyond the list's last; here the
    merge ends there.  It also sorts the files by name and compares stems, so `a-1.wav` in front of `a.wav` hides `a`; here the
    files are sorted by stem, which a directory in front of the name (--recursive) does not disturb either.
  * The suffix is compared without regard to case (`--file_extension .WAV` reads `x.wav` and `x.WAV`).
  * A file already at the target rate is re-encoded on the host without a kernel launch.
"""
import argparse
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch

from ... import audio

SUPPORTED = (".wav", ".flac")
PACK_BYTES = 1 << 30            # float32 input samples uploaded and converted per launch


def get_names_list(path_tsv_file):
    """First column of every non-empty line of the phone file."""
    with open(path_tsv_file, "r") as file:
        return [line.split()[0] for line in file if line.split()]


def check_extension(extension):
    if extension.lower() == ".mp3":
        raise ValueError("--file_extension .mp3: there is no mp3 decoder in this package; decode the files to .wav or .flac first")
    if extension.lower() not in SUPPORTED:
        raise ValueError(f"--file_extension {extension}: only {' and '.join(SUPPORTED)} files can be read")


def list_files(path_db, extension, recursive=False):
    """Relative paths of the files with the suffix (compared without regard to case, as check_extension reads it): the flat
    listing, or the whole tree."""
    def matches(name):
        return Path(name).suffix.lower() == extension.lower()

    if not recursive:
        return [f for f in os.listdir(path_db) if matches(f) and os.path.isfile(os.path.join(path_db, f))]
    found = []
    for root, _dirs, files in os.walk(path_db):
        rel = os.path.relpath(root, path_db)
        found += [f if rel == "." else os.path.join(rel, f) for f in files if matches(f)]
    return found


def select_files(file_list_db, file_list_phone):
    """Files whose stem is in the phone list.  Both lists are sorted by stem (the files by (stem, path): the merge compares stems,
    and neither a directory in front of a name nor the suffix behind it follows the stems' order) and merged in one pass that ends
    with the shorter of the two; files that share a stem are all taken.  file_list_phone None: every file, in the same order."""
    files = sorted(file_list_db, key=lambda f: (Path(f).stem, f))
    if file_list_phone is None:
        return files
    phones = sorted(file_list_phone)
    out_list, index_phone = [], 0
    for file_name in files:
        stem = Path(file_name).stem
        while index_phone < len(phones) and stem > phones[index_phone]:
            index_phone += 1
        if index_phone >= len(phones):
            break
        if stem == phones[index_phone]:
            out_list.append(file_name)
    return out_list


def require_device():
    """The device the conversion runs on; without one the tool refuses as the rest of the package does."""
    if not torch.cuda.is_available():
        raise RuntimeError("cpc2_amd runs only on a GPU (HIP) device and none is available: adjust_sample_rate resamples and "
                           "quantises on the device. There is no CPU fallback.")
    return torch.device("cuda", torch.cuda.current_device())


def _out_path(path_db_out, item):
    return os.path.join(path_db_out, str(Path(item).with_suffix(".wav")))


def _host_pcm16(wav):
    v = np.rint(wav.numpy() * np.float32(32768.0))
    return np.clip(v, -32768, 32767).astype(np.int16), int(((v < -32768) | (v > 32767)).sum())


def _convert_pack(pack, rate, target_sr, path_db_out, device, timings):
    """pack: [(item, waveform [channels, samples] on the host)] at one source rate."""
    def lap(stage, t0):
        if timings is not None:
            torch.cuda.synchronize(device)
            timings[stage] = timings.get(stage, 0.0) + time.perf_counter() - t0
        return time.perf_counter()

    t0 = time.perf_counter()
    lengths = [wav.shape[1] for _item, wav in pack for _c in range(wav.shape[0])]
    flat = torch.cat([wav.reshape(-1) for _item, wav in pack]).to(device)
    t0 = lap("upload", t0)
    o, n, _w, _taps = audio.resample_plan(rate, target_sr)
    dense = torch.empty(sum(audio.output_length(v, o, n) for v in lengths), dtype=torch.float32, device=device)
    outs = audio.resample_pack(flat, rate, target_sr, lengths=lengths, out=dense)          # (dense: the results follow one another)
    t0 = lap("kernel", t0)
    q, clamped = audio.to_pcm16(dense)
    q = q.cpu()
    t0 = lap("quantise", t0)
    at, k = 0, 0
    for item, wav in pack:
        channels, n_out = wav.shape[0], outs[k].numel()
        audio.write_wav(_out_path(path_db_out, item), q[at:at + channels * n_out].view(channels, n_out), target_sr)
        at += channels * n_out
        k += channels
    lap("write", t0)
    return int(clamped.item())


def adjust_sample_rate(path_db, file_list, path_db_out, target_sr, device=None, pack_bytes=PACK_BYTES, timings=None):
    """Converts file_list (paths relative to path_db) to target_sr under path_db_out; returns the number of clamped samples.
    Files are grouped by their rate (read from the headers), a group is cut into packs of at most pack_bytes of float32 input,
    and a pack is one upload, one resampling launch, one quantisation and one download.  timings: a dict that receives the
    seconds spent in decode / upload / kernel / quantise / write (the device is then synchronised between the stages)."""
    device = require_device() if device is None else torch.device(device)
    by_rate = {}
    for item in file_list:
        by_rate.setdefault(audio.info(os.path.join(path_db, item))[0], []).append(item)
    clamped = 0
    for rate in sorted(by_rate):
        pack, held = [], 0
        for item in by_rate[rate]:
            t0 = time.perf_counter()
            wav, _sr = audio.load(os.path.join(path_db, item))
            wav = wav.float()
            os.makedirs(os.path.dirname(_out_path(path_db_out, item)) or ".", exist_ok=True)
            if timings is not None:
                timings["decode"] = timings.get("decode", 0.0) + time.perf_counter() - t0
            if rate == target_sr:
                q, n_clamped = _host_pcm16(wav)
                audio.write_wav(_out_path(path_db_out, item), q, target_sr)
                clamped += n_clamped
                continue
            if pack and held + 4 * wav.numel() > pack_bytes:
                clamped += _convert_pack(pack, rate, target_sr, path_db_out, device, timings)
                pack, held = [], 0
            pack.append((item, wav))
            held += 4 * wav.numel()
        if pack:
            clamped += _convert_pack(pack, rate, target_sr, path_db_out, device, timings)
    return clamped


def parse_args(argv):
    parser = argparse.ArgumentParser(description="Adjust the sample rate of a given group of audio files")
    parser.add_argument("path_db", type=str, help="Path to the directory containing the audio files")
    parser.add_argument("path_phone_files", type=str, nargs="?", default=None,
                        help="Path to the .txt file containing the list of the files with a phone transcription "
                        "(left out: every file is converted)")
    parser.add_argument("path_out", type=str, help="Path to the output directory")
    parser.add_argument("--out_sample_rate", type=int, default=16000, help="Sample rate of the output audio files (default 16000)")
    parser.add_argument("--file_extension", type=str, default=".wav", help="Suffix of the input files: .wav (default) or .flac")
    parser.add_argument("--recursive", action="store_true", help="Walk the sub-directories of path_db and mirror them under path_out")
    return parser.parse_args(argv)


def main(argv):
    args = parse_args(argv)
    check_extension(args.file_extension)
    if args.out_sample_rate <= 0:
        raise ValueError(f"--out_sample_rate {args.out_sample_rate}: give a positive rate")
    if os.path.exists(args.path_out) and (not os.path.isdir(args.path_out) or os.listdir(args.path_out)):
        raise ValueError(f"path_out {args.path_out} exists and is not empty: nothing is overwritten, give a new directory")

    device = require_device()                                          # (before anything is read or created)

    file_list_db = list_files(args.path_db, args.file_extension, args.recursive)
    print(f"Found {len(file_list_db)} in the dataset")
    file_list_phone = None
    if args.path_phone_files is not None:
        file_list_phone = get_names_list(args.path_phone_files)
        print(f"Found {len(file_list_phone)} with a phone transcription")
    out_list = select_files(file_list_db, file_list_phone)
    print(f"Converting {len(out_list)} files")
    outputs = {}
    for item in out_list:                                              # (x.wav and x.WAV both become x.wav)
        other = outputs.setdefault(_out_path(args.path_out, item), item)
        if other != item:
            raise ValueError(f"{other} and {item} would both be written to {_out_path(args.path_out, item)}: nothing is overwritten")

    Path(args.path_out).mkdir(parents=True, exist_ok=True)
    clamped = adjust_sample_rate(args.path_db, out_list, args.path_out, args.out_sample_rate, device=device)
    print(f"Clamped {clamped} samples to the 16-bit range")
    return clamped


if __name__ == "__main__":
    main(sys.argv[1:])
