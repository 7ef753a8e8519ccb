#!/usr/bin/env python3
"""Timings of the whole-utterance CTC phone recogniser on one MI355X ("Common Voice phone recognition").  Prints one
JSON object and writes it to --out.  Times only: nothing here is a promise.

  1. The head -- seqNorm over the first len frames, the strided classifier and CTC with input lengths, forward and backward --
     on the library (cpc2_amd.eval.common_voices_eval.CTCphone_criterion) against the same head in plain torch on the device
     (the reference's per-utterance mean / var loop, nn.Conv1d, log_softmax + nn.CTCLoss with input lengths): device events
     around one forward + backward, the two arms taken in turn for --rounds rounds; median, minimum and maximum per arm.
     Features [8, 1500, 256] (15 s utterances), 41 phones, 120 labels per utterance.
  2. One `train` epoch (--freeze) and one `per` pass over the nine utterances of tests/golden/test_db with the recorded CPC
     checkpoint, by stage (the device is synchronised between the stages): wall seconds.

    python tools/common_voice_bench.py [--rounds 15] [--out profiles/common_voice_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cpc2_amd.dataset import findAllSeqs, parseSeqLabels  # noqa: E402
from cpc2_amd.eval import common_voices_eval as cv  # noqa: E402
from cpc2_amd.feature_loader import loadModel  # noqa: E402
from cpc2_amd.seq_alignment import beam_search_batch, get_seq_PER_batch  # noqa: E402

DEV = torch.device("cuda:0")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), rounds=len(ms))


class TorchHead(torch.nn.Module):
    """The reference's CTCphone_criterion (seqNorm, no LSTM) with integer lengths, on torch's own kernels."""

    def __init__(self, crit):
        super().__init__()
        self.conv = torch.nn.Conv1d(crit.PhoneCriterionClassifier.in_channels, crit.PhoneCriterionClassifier.out_channels, 8, stride=4)
        self.conv.load_state_dict(crit.PhoneCriterionClassifier.state_dict())
        self.loss = torch.nn.CTCLoss(blank=crit.BLANK_LABEL, reduction="mean", zero_infinity=True)

    def forward(self, c, sizes, label, label_size):
        rows = []
        for b in range(c.size(0)):
            n = int(sizes[b])
            m = c[b, :n].mean(dim=0, keepdim=True)
            v = c[b, :n].var(dim=0, keepdim=True)
            rows.append((c[b] - m) / torch.sqrt(v + 1e-8))
        pred = self.conv(torch.stack(rows).permute(0, 2, 1)).permute(2, 0, 1)
        in_len = torch.clamp(sizes // 4, max=pred.size(0))
        return self.loss(torch.log_softmax(pred, 2), label, in_len, label_size)


def head(rounds):
    b, s, h, n_phones, n_labels = 8, 1500, 256, 41, 120
    g = torch.Generator().manual_seed(0)
    c = torch.randn(b, s, h, generator=g).to(DEV).requires_grad_()
    sizes_host = [1500, 1433, 1201, 987, 1500, 760, 1322, 1111]
    sizes = torch.tensor(sizes_host, device=DEV)
    label = torch.randint(0, n_phones, (b, n_labels), generator=g).to(DEV)
    label_size = torch.full((b,), n_labels, device=DEV)
    torch.manual_seed(0)
    crit = cv.CTCphone_criterion(h, n_phones, seqNorm=True, reduction="mean").to(DEV)
    plain = TorchHead(crit).to(DEV)

    def ours():
        c.grad = None
        crit.zero_grad(set_to_none=True)
        crit(c, sizes, label, label_size).mean().backward()

    def torch_arm():
        c.grad = None
        plain.zero_grad(set_to_none=True)
        plain(c, sizes, label, label_size).backward()

    arms = {"library": ours, "plain_torch": torch_arm}
    for fn in arms.values():
        fn()
        fn()
    torch.cuda.synchronize()
    loss_a = float(crit(c, sizes, label, label_size))
    loss_b = float(plain(c, sizes, label, label_size))
    ms = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            ms[k].append(once(fn))
    out = {k: stats(v) for k, v in ms.items()}
    out.update(shape=[b, s, h], phones=n_phones, labels=n_labels, loss_library=loss_a, loss_plain_torch=loss_b)
    return out


class Laps:
    def __init__(self):
        self.s = {}
        self.t0 = time.perf_counter()

    def lap(self, stage):
        torch.cuda.synchronize()
        now = time.perf_counter()
        self.s[stage] = self.s.get(stage, 0.0) + now - self.t0
        self.t0 = now


def tool():
    ckpt = os.path.join(GOLDEN, "ref_checkpoint", "checkpoint_7.pt")
    laps = Laps()
    labels, n_phones = parseSeqLabels(os.path.join(GOLDEN, "g27_phone_transcripts.txt"))
    seqs, _ = findAllSeqs(os.path.join(GOLDEN, "test_db"), extension=".flac")
    model, hidden, _ = loadModel([ckpt])
    model.to(DEV).eval()
    model.optimize = False
    for p in model.parameters():
        p.requires_grad = False
    torch.manual_seed(0)
    crit = cv.CTCphone_criterion(hidden, n_phones, reduction="mean").to(DEV)
    ds = cv.SingleSequenceDataset(os.path.join(GOLDEN, "test_db"), seqs, labels, random_offset_amplitude=0)
    opt = torch.optim.AdamW(list(crit.parameters()), lr=2e-4)
    laps.lap("load")
    out = {}
    for rep in range(2):                               # the second pass is the record (the first loads code objects)
        train = Laps()
        crit.train()
        for data in ds.batches(4, shuffle=True):
            seq, size_seq, phone, size_phone = cv.prepare_data(data)
            train.lap("batch")
            with torch.no_grad():
                c = model(seq, None)[0]
            train.lap("features")
            opt.zero_grad()
            loss = crit(c, size_seq // 160, phone, size_phone)
            loss.mean().backward()
            train.lap("head_forward_backward")
            opt.step()
            train.lap("optimizer")
        crit.eval()
        pers = []
        per = Laps()                                     # (started here: its first lap is the first batch, not the train epoch)
        for data in ds.batches(4, shuffle=False):
            seq, size_seq, phone, size_phone = cv.prepare_data(data)
            per.lap("batch")
            with torch.no_grad():
                c = model(seq, None)[0]
                per.lap("features")
                frames = size_seq // 160
                probs = torch.softmax(crit.getPrediction(c, frames), dim=2)
                per.lap("predictions")
                lengths = torch.clamp(frames // 4, max=probs.size(1))
                _, found_sizes, found, _, ties = beam_search_batch(probs, lengths, 20, crit.BLANK_LABEL, best_only=True)
                pers.append(torch.stack([get_seq_PER_batch(phone, size_phone, found[:, 0], found_sizes[:, 0]), ties.double()]).cpu())
                per.lap("search_and_score")
        out = dict(train_epoch_s=train.s, per_pass_s=per.s, utterances=len(ds), batch=4, frames_max=int(ds.maxSize // 160),
                   mean_per=float(torch.cat(pers, 1)[0].mean()))
    out["load_s"] = laps.s["load"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "common_voice_bench.json"))
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "head": head(args.rounds), "tool": tool()}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=2)


if __name__ == "__main__":
    main()
