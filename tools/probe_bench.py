#!/usr/bin/env python3
"""Timings of the linear-separability probe on one MI355X.  Prints one JSON object and writes it to
--out.

  1. cross-entropy head, forward + backward (logits GEMM with bias, cpc_probe_xent, dW / db / dX) against plain torch
     (F.linear + F.cross_entropy + max + backward) at N in {8*128, 64*128}, C in {41, 251, 2338}, H in {256, 512};
  2. CTC, forward + backward from given logits (cpc_probe_ctc + the scale pass) against torch.nn.functional.ctc_loss on
     log_softmax at B in {8, 64}, T = 128, K = 42, target lengths 15-40 (collapsed phone labels) and 128;
  3. one frozen probe epoch of CPC-small (encoder 256 + GRU 256) on synthetic audio, batch 8: ms per batch, split into the
     feature extraction and the probe (PhoneCriterion forward + backward + FlatAdam step).

    python tools/probe_bench.py [--quick] [--out profiles/probe_bench.json]
Times are device events around --iters repetitions after --warmup ones; the kernel statistics come from a separate
`rocprofv3 --kernel-trace --stats` run of this script with --quick.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cpc2_amd import _lib  # noqa: E402
from cpc2_amd.criterion import PhoneCriterion, _ProbeHeadFn  # noqa: E402
from cpc2_amd.train import FlatAdam  # noqa: E402

DEV = torch.device("cuda:0")
HBM_BYTES_PER_S = 8.0e12          # MI355X HBM3E peak (MI355X_MICROARCH.md)


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


def xent_case(n, c, h, warmup, iters):
    g = torch.Generator(device=DEV).manual_seed(n + c + h)
    x = torch.randn(n, h, device=DEV, generator=g).requires_grad_(True)
    w = (torch.randn(c, h, device=DEV, generator=g) / h ** 0.5).requires_grad_(True)
    b = torch.zeros(c, device=DEV).requires_grad_(True)
    y = torch.randint(0, c, (n,), device=DEV, generator=g)

    def ours():
        x.grad = w.grad = b.grad = None
        loss, acc = _ProbeHeadFn.apply(x, w, b, "xent", y, None, False, True)
        loss.sum().backward()

    def plain():
        x.grad = w.grad = b.grad = None
        z = torch.nn.functional.linear(x, w, b)
        loss = torch.nn.functional.cross_entropy(z, y)
        (z.max(1)[1] == y).double().mean()
        loss.backward()

    t_ours, t_plain = timed(ours, warmup, iters), timed(plain, warmup, iters)
    logits_bytes = 4 * n * c
    return dict(N=n, C=c, H=h, ours_ms=t_ours, torch_ms=t_plain, speedup=t_plain / t_ours, logits_bytes=logits_bytes,
                # the row pass reads the logits once and writes dlogits once: its floor at peak HBM bandwidth
                row_pass_floor_us=2 * logits_bytes / HBM_BYTES_PER_S * 1e6)


def ctc_case(B, L_lo, L_hi, warmup, iters, T=128, K=42):
    lib = _lib.load()
    rng = np.random.default_rng(B * 100 + L_lo)
    lengths = rng.integers(L_lo, L_hi + 1, size=B)
    padded = np.zeros((B, T), np.int64)
    for i, L in enumerate(lengths):
        tg = rng.integers(0, K - 1, size=L)
        if L == T:                                 # keep the all-frames case feasible: no equal neighbours
            tg = (np.arange(T) + i) % (K - 1)
        padded[i, :L] = tg
    logits = torch.randn(B, T, K, device=DEV) * 2
    tg = torch.from_numpy(padded).to(DEV)
    ln = torch.from_numpy(lengths.astype(np.int64)).to(DEV)
    nll = torch.empty(B, device=DEV)
    loss = torch.empty(1, device=DEV)
    dl = torch.empty_like(logits)
    one = torch.ones(1, device=DEV)
    nb = lib.cpc_probe_ctc_scratch_bytes(B, T, T)
    sc = torch.empty(nb, dtype=torch.uint8, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def ours():
        _lib.check(lib.cpc_probe_ctc(p(logits), B, T, K, p(tg), T, p(ln), p(nll), p(loss), p(dl), p(sc), nb, st), "probe_ctc")
        _lib.check(lib.cpc_probe_head_backward(p(dl), B * T, K, p(one), None, None, 0, st), "probe_head_backward")

    flat = torch.cat([tg[i, :int(lengths[i])] for i in range(B)])
    il = torch.full((B,), T, dtype=torch.long, device=DEV)
    x = logits.clone().requires_grad_(True)

    def plain():
        x.grad = None
        lp = torch.log_softmax(x, dim=2).permute(1, 0, 2)
        torch.nn.functional.ctc_loss(lp, flat, il, ln, blank=K - 1, reduction="mean", zero_infinity=True).backward()

    t_ours, t_plain = timed(ours, warmup, iters), timed(plain, warmup, iters)
    return dict(B=B, T=T, K=K, L=[int(L_lo), int(L_hi)], ours_ms=t_ours, torch_ms=t_plain, speedup=t_plain / t_ours,
                ours_us_per_frame_step=t_ours * 1e3 / (2 * T))


def epoch_case(n_batches, warmup):
    import cpc2_amd
    from oracle import synth
    hidden, b = 256, 8
    mp = synth.encoder_params(hidden, 21)
    mp.update(synth.gru_params(hidden, hidden, 1, 22))
    model = cpc2_amd.CPCModel(cpc2_amd.CPCEncoder(hidden), cpc2_amd.CPCAR(hidden, hidden, False, 1))
    model.load_state_dict(mp)
    model = model.to(DEV).eval()
    for prm in model.parameters():
        prm.requires_grad = False
    torch.manual_seed(0)
    crit = PhoneCriterion(hidden, 41, False).to(DEV)
    opt = FlatAdam(list(crit.parameters()), lr=2e-4, eps=2e-8)
    xs = [synth.audio_windows(b, 20480, 100 + i).to(DEV) for i in range(4)]
    labels = [torch.randint(0, 41, (b, 128), device=DEV) for _ in range(4)]
    feats = []

    def extract(i):
        with torch.no_grad():
            c, _, _ = model(xs[i % 4], None)
        return c

    def probe(c, i):
        opt.zero_grad()
        loss, acc = crit(c, c, labels[i % 4])
        loss.sum().backward()
        opt.step()
        return loss, acc

    for i in range(warmup):
        probe(extract(i), i)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    t_feat = t_probe = 0.0
    for i in range(n_batches):
        ev[0].record()
        c = extract(i)
        ev[1].record()
        out = probe(c, i)
        ev[2].record()
        feats.append(out[0].detach())
        torch.cuda.synchronize()
        t_feat += ev[0].elapsed_time(ev[1])
        t_probe += ev[1].elapsed_time(ev[2])
    return dict(batch=b, hidden=hidden, batches=n_batches, features_ms_per_batch=t_feat / n_batches,
                probe_ms_per_batch=t_probe / n_batches, total_ms_per_batch=(t_feat + t_probe) / n_batches,
                probe_share=t_probe / (t_feat + t_probe))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="one size of each kind, few repetitions (for the profiler run)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_bench needs the GPU")
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "torch_ctc_backend": "ATen native GPU kernel (ctc_loss_gpu): MIOpen's CTC is used only with blank 0, int32 "
                                "targets and every input length equal, and blank here is K - 1",
           "cudnn_enabled": torch.backends.cudnn.enabled}
    if args.quick:
        res["xent"] = [xent_case(8 * 128, 41, 256, 2, 5)]
        res["ctc"] = [ctc_case(8, 15, 40, 2, 5)]
        res["epoch"] = epoch_case(5, 2)
    else:
        res["xent"] = [xent_case(n, c, h, args.warmup, args.iters) for n in (8 * 128, 64 * 128) for c in (41, 251, 2338)
                       for h in (256, 512)]
        res["ctc"] = [ctc_case(B, lo, hi, args.warmup, args.iters) for B in (8, 64) for lo, hi in ((15, 40), (128, 128))]
        res["epoch"] = epoch_case(40, args.warmup)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
