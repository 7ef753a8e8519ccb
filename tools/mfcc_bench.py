#!/usr/bin/env python3
"""The log-mel / MFCC kernels (csrc/mfcc.hip) and the tool build_baseline_features on one MI355X.  Writes
profiles/mfcc_bench.json (and prints it).

Kernels: one pack of 360 signals of 10 s less half a hop (one hour at 16 kHz, 360 000 frames) in two configurations -- the tool's default
(n_fft 400, 40 mels, 13 coefficients) and the reference's MFCCEncoder(256)-sized one (n_fft 321, 128 mels, 64 coefficients).  Per
configuration, timed by device events in alternating rounds (kernels, torch f32, torch f64, kernels, ...), the best round and the
spread (max / min over the rounds) of each:
  kernel_ms         MFCC.__call__ on the pack: cpc_melspec_db + cpc_mfcc_finish (table upload and scratch already there)
  torch_f32_ms      the plain-torch restatement on the device: torch.stft (reflect, periodic Hann) -> |.|^2 -> @ fb -> dB with the
  torch_f64_ms      per-signal floor -> @ dct, on a [360, 159920] batch, in float32 and in float64 (the f64 one converts the
                    samples first: 8 bytes per sample the kernels never write)
  bytes_floor_ms    the samples read once and the f32 result written once at 8.0 TB/s (HBM3E spec)
  flops_floor_ms    the windowed DFT's 2 * 2 * n_fft * n_freqs flops per frame (the plain form; the kernel folds the samples n and
                    n_fft - n first and issues half of them) at the f64 matrix rate of tools/mfma_f64_probe.hip
                    (75.09 TFLOP/s, profiles/cca_bench.json; --probe_tflops to restate it)
  issued_tflops     the flops of the padded tiles the kernels actually run (DFT and filterbank products) over kernel_ms
  max_abs_difference_to_torch_f64   the two f64 computations agree to this (largest element, dB / coefficient units)
Tool: python -m cpc2_amd.eval.build_baseline_features on the same synthetic hour written as 360 wav files, seconds by stage.

    python tools/mfcc_bench.py [--reps 5] [--rounds 3] [--no-tool]
"""
import argparse
import json
import math
import os
import shutil
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cpc2_amd import spectral  # noqa: E402

HBM_BPS = 8.0e12
DEV = torch.device("cuda:0")
CONFIGS = [dict(n_fft=400, hop=160, n_mels=40, n_mfcc=13), dict(n_fft=321, hop=160, n_mels=128, n_mfcc=64)]
FILES, SECONDS = 360, 10


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(reps):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / reps


def torch_restatement(x, t, dtype):
    """The definition in plain torch on the device, grid "center" (what torch.stft's own centring gives)."""
    host = spectral.host_tables(t.n_fft, t.n_mels, t.n_out, t.sample_rate)
    Wp, F = (t.n_fft + 3) // 4 * 4, t.n_fft // 2 + 1
    Hp, Fp, Mp = (F + 3) // 4 * 4, (F + 15) // 16 * 16, (t.n_mels + 15) // 16 * 16
    o = Wp + 2 * Hp * Fp
    fb = host[o:o + Fp * Mp].view(Fp, Mp)[:F, :t.n_mels].to(DEV, dtype)
    dct = host[o + Fp * Mp:].view(t.n_mels, t.n_out).to(DEV, dtype)
    window = host[:t.n_fft].to(DEV, dtype)

    def run():
        spec = torch.stft(x.to(dtype), t.n_fft, hop_length=t.hop, window=window, center=True, pad_mode="reflect", return_complex=True)
        power = spec.real ** 2 + spec.imag ** 2                              # [b, F, T]
        mel = power.transpose(1, 2) @ fb
        db = 10.0 * torch.log10(mel.clamp_min(1e-10))
        db = torch.maximum(db, db.amax(dim=(1, 2), keepdim=True) - t.top_db)
        return db @ dct
    return run


def config_record(cfg, reps, rounds, probe_tflops):
    gen = torch.Generator().manual_seed(cfg["n_fft"])
    length = SECONDS * 16000 - 80          # not a multiple of the hop: torch.stft with an odd n_fft then has our 1 + L // hop frames
    x = (0.1 * torch.randn(FILES, length, generator=gen)).to(DEV)
    t = spectral.MFCC(grid="center", **cfg)
    frames = FILES * t.n_frames(length)
    flat, lengths = x.view(-1), [length] * FILES
    out = torch.empty(frames, t.n_out, dtype=torch.float32, device=DEV)

    def mine():
        return t(flat, lengths=lengths, out=out)

    base32, base64 = torch_restatement(x, t, torch.float32), torch_restatement(x, t, torch.float64)
    mine()
    ref = base64()
    n_ref = ref.size(1)                                                      # torch.stft: 1 + (L + 2 (n_fft // 2) - n_fft) // hop frames
    got = out.view(FILES, -1, t.n_out)[:, :n_ref].double()
    diff64 = float((got - ref).abs().max())
    diff32 = float((base32().double() - ref).abs().max())
    del ref, got
    a, b, c = [], [], []
    for _ in range(rounds):
        a.append(timed(mine, reps))
        b.append(timed(base32, reps))
        c.append(timed(base64, reps))
    F = t.n_fft // 2 + 1
    Hp, Fp, Mp = (F + 3) // 4 * 4, (F + 15) // 16 * 16, (t.n_mels + 15) // 16 * 16
    tiles = FILES * math.ceil(t.n_frames(length) / spectral.FRAME_TILE)
    issued = 2.0 * tiles * spectral.FRAME_TILE * (Hp * 2 * Fp + Fp * Mp)
    dft = 2.0 * frames * t.n_fft * 2 * F
    return dict(cfg, files=FILES, samples=FILES * length, frames=frames, kernel_ms=min(a), kernel_spread=max(a) / min(a),
                torch_f32_ms=min(b), torch_f32_spread=max(b) / min(b), torch_f64_ms=min(c), torch_f64_spread=max(c) / min(c),
                kernel_over_torch_f32=min(a) / min(b), kernel_over_torch_f64=min(a) / min(c),
                bytes_floor_ms=(4.0 * FILES * length + 4.0 * frames * t.n_out) / HBM_BPS * 1e3,
                flops_floor_ms=dft / (probe_tflops * 1e12) * 1e3, issued_tflops=issued / (min(a) * 1e-3) / 1e12,
                frac_of_probe_rate=issued / (min(a) * 1e-3) / 1e12 / probe_tflops,
                scratch_bytes=int(spectral._lib.load().cpc_melspec_scratch_bytes(tiles, FILES, t.n_mels)),
                torch_f64_frames_compared=n_ref * FILES, max_abs_difference_to_torch_f64=diff64,
                max_abs_difference_torch_f32_to_f64=diff32)


def tool_record():
    from cpc2_amd import audio
    from cpc2_amd.eval import build_baseline_features as B
    tmp = tempfile.mkdtemp()
    try:
        gen = torch.Generator().manual_seed(0)
        os.makedirs(os.path.join(tmp, "db", "spk"))
        for i in range(FILES):
            wave = (0.1 * torch.randn(1, SECONDS * 16000, generator=gen)).clamp(-1, 1)
            audio.write_wav(os.path.join(tmp, "db", "spk", f"f{i:04d}.wav"), (wave * 32767).round().to(torch.int16), 16000)
        t0 = time.perf_counter()
        timings = B.main([os.path.join(tmp, "db"), os.path.join(tmp, "out")])
        wall = time.perf_counter() - t0
        return dict(files=FILES, audio_s=FILES * SECONDS, format="pt", columns=39, wall_s=wall,
                    stage_s={k: round(v, 4) for k, v in timings.items()})
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--probe_tflops", type=float, default=75.09, help="f64 matrix rate of tools/mfma_f64_probe.hip on this device")
    ap.add_argument("--no-tool", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mfcc_bench.json"))
    a = ap.parse_args()
    out = dict(device=torch.cuda.get_device_name(0), probe_tflops=a.probe_tflops, hbm_bytes_per_s=HBM_BPS, configs=[])
    t0 = time.perf_counter()
    for cfg in CONFIGS:
        out["configs"].append(config_record(cfg, a.reps, a.rounds, a.probe_tflops))
    if not a.no_tool:
        out["tool"] = tool_record()
    out["wall_s"] = time.perf_counter() - t0
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
