#!/usr/bin/env python3
"""Timings of the audio augmentation on one MI355X.  Prints one JSON object and writes it to --out.

  1. the mix kernel (cpc_augment_additive, speech and noise windows read by offset out of flat vectors) at b = 64,
     W = 20480 beside a plain-torch restatement (gather + elementwise ops) and beside its floor: the bytes it has to move
     (two windows read, one written) at the HBM rate;
  2. the FIR (cpc_augment_fir: direct form + peak normalisation) at response lengths 257 .. 16000 beside a torch.fft
     restatement (rfft / irfft of the batch, cut to W, peak normalisation) and beside its floor: the multiply-adds the causal
     truncated convolution needs at the f32 FMA rate;
  3. cpc2_amd.train.trainStep on the window feeder at CPC-small, b = 64, files from disk as bench.py's small_feeder
     configuration reads them, for --augment_type none / additive / natural_reverb (0.5 s and 1 s responses) / additive
     natural_reverb on the past half.  The arms ALTERNATE, epoch by epoch, inside this one process on this one box; a figure
     is the median over the rounds, with the spread beside it.

    python tools/augment_bench.py [--quick] [--out profiles/augment_bench.json]
Kernel times are device events around --iters repetitions after --warmup ones."""
import argparse
import contextlib
import io
import json
import os
import random
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cpc2_amd import _lib  # noqa: E402
from cpc2_amd import data_augmentation as da  # noqa: E402
from cpc2_amd._lib import check, ptr, stream_ptr  # noqa: E402

DEV = torch.device("cuda:0")
HBM_BYTES_PER_S = 8.0e12          # MI355X HBM3E peak (MI355X_MICROARCH.md); 6.3e12 is what a copy achieves
F32_FLOPS = 157.3e12              # peak f32 vector rate (spec, with packed f32; this library builds without packed f32: half of it)
W = 20480


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def mix_case(b, warmup, iters):
    g = torch.Generator(device=DEV).manual_seed(b)
    speech = torch.randn(400 * W, device=DEV, generator=g) * 0.05
    noise = torch.randn(100 * W, device=DEV, generator=g) * 0.1
    s_off = torch.randint(0, speech.numel() - W, (b,), device=DEV, generator=g)
    n_off = torch.randint(0, noise.numel() - W, (b,), device=DEV, generator=g)
    gain = torch.rand(b, device=DEV, generator=g) * 0.5 + 0.1
    out = torch.empty(b, W, device=DEV)
    lib, st = _lib.load(), stream_ptr(DEV)
    ar = torch.arange(W, device=DEV)

    def ours():
        check(lib.cpc_augment_additive(ptr(speech), speech.numel(), ptr(s_off), ptr(noise), noise.numel(), ptr(n_off), 1, ptr(gain),
                                       ptr(out), b, W, st), "augment_additive")

    def plain():
        x = speech[s_off.unsqueeze(1) + ar]
        n = noise[n_off.unsqueeze(1) + ar]
        n = n / (n.abs().max(dim=1, keepdim=True)[0] + 1e-8)
        ex = x / (torch.sqrt(torch.mean(x ** 2, dim=1, keepdim=True)) + 1e-8)
        en = n / (torch.sqrt(torch.mean(n ** 2, dim=1, keepdim=True)) + 1e-8)
        m = ex + en * gain.unsqueeze(1)
        return m / (m.abs().max(dim=1, keepdim=True)[0] + 1e-8)

    ours()
    err = float((out - plain()).abs().max())
    t_ours, t_plain = timed(ours, warmup, iters), timed(plain, warmup, iters)
    nbytes = 3 * 4 * b * W
    floor_us = nbytes / HBM_BYTES_PER_S * 1e6
    return dict(b=b, W=W, ours_us=t_ours * 1e3, torch_us=t_plain * 1e3, speedup=t_plain / t_ours, bytes=nbytes,
                floor_us=floor_us, share_of_floor=floor_us / (t_ours * 1e3), bound="HBM bytes", max_abs_diff_vs_torch=err)


def fir_case(b, length, warmup, iters):
    g = torch.Generator(device=DEV).manual_seed(length)
    x = torch.randn(b, W, device=DEV, generator=g) * 0.05
    t = torch.arange(length, device=DEV, dtype=torch.float32)
    irs = torch.randn(b, length, device=DEV, generator=g) * torch.exp(-t / (length / 6.0))
    flat = irs.reshape(-1).contiguous()
    off = (torch.arange(b, device=DEV) * length).to(torch.int64)
    ln = torch.full((b,), length, dtype=torch.int32, device=DEV)
    out = torch.empty_like(x)
    lib, st = _lib.load(), stream_ptr(DEV)
    need = lib.cpc_augment_fir_scratch_bytes(b, W)
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    n_fft = 1 << int(np.ceil(np.log2(W + length - 1)))

    def ours():
        check(lib.cpc_augment_fir(ptr(x), ptr(flat), flat.numel(), ptr(off), ptr(ln), ptr(out), ptr(scratch), need, b, W, st), "augment_fir")

    def plain():
        y = torch.fft.irfft(torch.fft.rfft(x, n_fft) * torch.fft.rfft(irs, n_fft), n_fft)[:, :W]
        return y / (y.abs().max(dim=1, keepdim=True)[0] + 1e-8)

    ours()
    err = float((out - plain()).abs().max())
    t_ours, t_plain = timed(ours, warmup, iters), timed(plain, warmup, iters)
    taps = min(length, W)
    macs = b * (W * taps - taps * (taps - 1) // 2)                 # sum over t of min(t + 1, L)
    floor_us = 2 * macs / F32_FLOPS * 1e6
    return dict(b=b, W=W, response=length, ours_us=t_ours * 1e3, torch_fft_us=t_plain * 1e3, speedup_vs_fft=t_plain / t_ours,
                multiply_adds=macs, achieved_tflops=2 * macs / (t_ours * 1e-3) / 1e12, floor_us=floor_us,
                share_of_floor=floor_us / (t_ours * 1e3), bound="f32 FMA rate (spec, packed)", max_abs_diff_vs_fft=err)


# ----------------------------------------------------------------------------- trainStep on the feeder
def write_wav(path, samples):
    import wave
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(path, "wb") as fh:
        fh.setnchannels(1)
        fh.setsampwidth(2)
        fh.setframerate(16000)
        fh.writeframes((np.clip(samples, -1, 1) * 32767).astype("<i2").tobytes())


def feeder_arms(batch, steps, rounds, quick):
    import bench
    from cpc2_amd.dataset import AudioBatchData, PeakNorm, findAllSeqs
    from cpc2_amd.train import DataParallelContext, trainStep
    cfg = bench.CONFIGS["small_feeder"]
    tmp = tempfile.mkdtemp(prefix="cpc_augment_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        bench.write_synthetic_corpus(os.path.join(tmp, "speech"), steps * batch, seed=7)
        bench.write_synthetic_corpus(os.path.join(tmp, "noise"), 40 * batch, n_speakers=2, files_per_speaker=8, seed=8)
        rng = np.random.RandomState(9)
        for tag, n in (("ir_half", 8000), ("ir_one", 16000)):
            for i in range(8):
                ir = rng.randn(n) * np.exp(-np.arange(n) / (n / 6.0)) * 0.3
                write_wav(os.path.join(tmp, tag, f"room_{i}.wav"), ir)
        random.seed(11)
        seqs, speakers = findAllSeqs(os.path.join(tmp, "speech"), extension=".wav")
        noise_seqs, _ = findAllSeqs(os.path.join(tmp, "noise"), extension=".wav", speaker_level=0)
        with contextlib.redirect_stdout(io.StringIO()):
            noise = AudioBatchData(os.path.join(tmp, "noise"), W, noise_seqs, None, 1, transform=PeakNorm(), device=DEV)
            kw = dict(noise_dataset=noise, additive_noise_snr_min=5.0, additive_noise_snr_max=20.0, batchSize=batch,
                      additive_noise_sampling="uniform", impulse_response_prob=1.0, ir_sample_rate=16000, ir_batch_wise=False, t_ms=100)
            half, one = os.path.join(tmp, "ir_half"), os.path.join(tmp, "ir_one")
            arms = {
                "none": None,
                "additive": da.get_augment("additive", **kw),
                "natural_reverb_0.5s": da.get_augment("natural_reverb", pathImpulseResponses=half, **kw),
                "natural_reverb_1s": da.get_augment("natural_reverb", pathImpulseResponses=one, **kw),
                "additive+natural_reverb_1s": da.CombinedTransforms(["additive", "natural_reverb"], pathImpulseResponses=one, **kw),
            }
            if quick:
                arms = {k: arms[k] for k in ("none", "additive+natural_reverb_1s")}
        import copy
        base = AudioBatchData(os.path.join(tmp, "speech"), W, seqs, None, len(speakers), device=DEV)
        data = {}
        for name, aug in arms.items():                              # one pack, resident once: the arms differ in the augmentation only
            data[name] = copy.copy(base)
            data[name].augment_past, data[name].augmentation = aug is not None, aug
        model, crit, opt = bench.build(cfg, DEV)
        dp = DataParallelContext(opt, early_params=list(crit.parameters()) + list(model.gAR.parameters()), timing=False)
        crit.seed(1234)
        crit.sampler.prefetch = True
        times = {name: [] for name in arms}

        def epoch(name):
            loader = data[name].getDataLoader(batch, "samespeaker", True)
            with contextlib.redirect_stdout(io.StringIO()):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                logs = trainStep(loader, model, crit, opt, None, 1000, dp=dp)
                torch.cuda.synchronize()
                return 1e3 * (time.perf_counter() - t0) / max(1, int(logs["iter"]))

        for name in arms:                                           # warm-up: whole epochs, every arm (first uses of every batch size)
            for _ in range(1 if quick else 2):
                epoch(name)
        for _ in range(rounds):
            for name in arms:                                       # alternating arms
                times[name].append(epoch(name))
        plan_us = {}
        for name in arms:                                           # the host side alone: a pack's sampler draws and its plan
            loader = data[name].getDataLoader(batch, "samespeaker", True)
            t0 = time.perf_counter()
            batches, _plans = loader.pack_plan()
            torch.cuda.synchronize()
            plan_us[name] = 1e6 * (time.perf_counter() - t0) / max(1, len(batches))
        _lib.check(_lib.load().cpc_async_error_check(stream_ptr(DEV)), "async error check")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    out = {}
    for name, ts in times.items():
        s = sorted(ts)
        out[name] = dict(ms_per_step_median=s[len(s) // 2], ms_per_step_min=s[0], ms_per_step_max=s[-1], rounds=len(s),
                         host_plan_us_per_step=plan_us[name])
    base = out["none"]["ms_per_step_median"]
    for name in out:
        out[name]["over_none_ms"] = out[name]["ms_per_step_median"] - base
    return dict(config="CPC-small (hidden 256, GRU, 12 predictions, 128 negatives)", batch=batch, steps_per_epoch=steps, arms=out,
                note="host clock around one epoch of trainStep ending in a device synchronise; the plan of the pack is drawn inside "
                     "the timed epoch, before its first step")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="one size of each kind, few repetitions")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--steps", type=int, default=200, help="steps per feeder epoch")
    ap.add_argument("--rounds", type=int, default=5, help="timed epochs per arm")
    ap.add_argument("--no_feeder", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench needs the GPU")
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__}
    if args.quick:
        res["mix"] = [mix_case(64, 2, 5)]
        res["fir"] = [fir_case(64, 4000, 2, 5)]
        if not args.no_feeder:
            res["feeder"] = feeder_arms(64, 40, 1, True)
    else:
        res["mix"] = [mix_case(b, args.warmup, args.iters) for b in (8, 64)]
        res["fir"] = [fir_case(64, n, args.warmup, args.iters) for n in (257, 4000, 8000, 16000)]
        if not args.no_feeder:
            res["feeder"] = feeder_arms(64, args.steps, args.rounds, False)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
