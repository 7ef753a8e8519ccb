"""Phone recognition on whole utterances of varying length (the reference's cpc/eval/common_voices_eval.py): a CTC head on the
features of a CPC checkpoint, trained on transcriptions that are not aligned (`train`) and scored by beam search (`per`).

    python -m cpc2_amd.eval.common_voices_eval train PATH_DB PATH_PHONE CHECKPOINT [-o OUT] [--freeze] [--pathTrain F] [--pathVal F]
                                               [--LSTM] [--seqNorm] [--dropout] [--loss_reduction mean|sum] [--roffset N] ...
    python -m cpc2_amd.eval.common_voices_eval per OUT [--name NAME] [--pathDB D] [--pathVal F] [--pathPhone F] [--batchSize B]
    python -m cpc2_amd.eval.common_voices_eval align OUT -o ALIGN_DIR [--pathDB D] [--pathVal F] [--pathPhone F] [--batchSize B]
                                               [--file_extension .wav] [--debug] [--blank_label N] [--name NAME]

Names and signatures are the reference's (SingleSequenceDataset, CTCphone_criterion, cut_data, prepare_data, train_step, val_step,
get_per, perStep, run, get_PER_args, both sub-commands with every flag).  The head runs on the library (include/cpc2_hip.h,
version 117): normalisation over the first `len` frames (cpc_seqnorm_len_*), the LSTM kernels, the strided classifier as the
products of cpc_gemm_nt (through cpc_conv_head_forward, which lends its K split room for an ordered sum) and cpc_gemm_tn over the
overlapping rows of the features plus cpc_conv_head_backward_data, and CTC with an input length per utterance (cpc_ctc_loss).  Audio is one resident device vector; a batch is one gather launch (cpc_gather_utterances).

The reference's CTCphone_criterion.forward does not run on a current torch (`featureSize /= 4` on an integer tensor raises, and
the float lengths that `sizeSeq / downsampling_factor` yields cannot index).  It was written for a torch whose `/` divided integer
tensors as integers, and that is what is computed here: frames = samples // 160, pred_len = min(frames // 4, P).

Deviations from the reference:
  * --file_extension defaults to .wav (the reference: .mp3).  There is no mp3 decoder: .mp3 is refused by name.
  * pathCheckpoint == "ID" (pre-computed .npy features) and --in_dim other than 1 are refused by name.
  * --augments is refused by name when given: it builds sox effect chains.
  * --kernelSize other than 8 is refused by name: the reference parses the flag and never hands it to the criterion, and a flag is
    not ignored silently here.  (CTCphone_criterion itself takes every even sizeKernel and divides the lengths by its stride,
    sizeKernel // 2, where the reference divides by 4 whatever the kernel size.)
  * One GPU per process, no DataParallel.  checkpoint.pt is written with the reference's `module.`-prefixed keys in `classifier`
    and `model`, so that the reference's `per` can load it; loading accepts keys with or without the prefix.
  * No `tee` subprocess and no dup2: logs_{command}{_name}.txt receives the lines that stdout receives.
  * getPrediction's seqNorm branch fills a buffer with torch.randn that it then overwrites whole; that draw from the generator is
    not reproduced.
  * A batch whose loss is not finite is skipped: no optimiser step, and it counts as 0 in the epoch's mean (the reference sets
    `loss = 0` and then dies in `.mean()`).
  * The batch order is a permutation from torch's global generator per epoch; it is not held to the DataLoader's order.  The
    items' random offsets are drawn with random.randint(0, random_offset_amplitude) in item order, as __getitem__ draws them.
  * perStep runs batched on the device (softmax, cpc_ctc_beam_search with 20 prefixes, cpc_align_score), one copy to the host per
    batch, no process pool and no progress bar; it also reports how many utterances met a tie in the search (seq_alignment.py).
  * `align` is not the reference's (it has no aligner): the trained head's best CTC alignment of every utterance with its
    transcription (cpc2_amd/seq_alignment.py: ctc_forced_align, whose docstring is the definition; cpc_ctc_align, version 120),
    written as one label per 10 ms frame (alignment_frames.txt, the format dataset.parseSeqLabels reads, so that
    linear_separability --pathPhone runs on a corpus that had no alignment), one line per token (alignment_segments.txt:
    name phone start_s end_s mean_log_posterior) and alignment_log.json.  One copy to the host per batch.  Agreement with
    torchaudio.functional.forced_align is UNMEASURED.  Writing ABX .item files from alignments is left as the follow-up: they
    need speaker and context columns, and a 40 ms grid is coarse for them.
All refusals happen before any audio file is looked for.
"""
import argparse
import contextlib
import ctypes
import io
import json
import math
import os
import random
import sys
import time
from copy import deepcopy
from pathlib import Path

import numpy as np
import torch

from .. import _lib, audio
from .._lib import check, f32c, ptr, require_gpu, scratch, stream_ptr
from ..dataset import filterSeqs, findAllSeqs, parseSeqLabels
from ..feature_loader import loadModel
from ..model import LSTMPredictor
from ..seq_alignment import (beam_search, beam_search_batch, ctc_forced_align, frame_labels, get_seq_PER, get_seq_PER_batch,
                             head_frame_of, head_tokens)

MAX_TARGET = 1024          # cpc_ctc_loss: labels per utterance (the extended states live in LDS)


# --------------------------------------------------------------------------- data
def load(path_item):
    """(stem, waveform [1, samples]) of one audio file; anything but one channel is refused."""
    path_item = Path(path_item)
    if path_item.suffix == '.npy':
        raise ValueError(f"{path_item}: pre-computed .npy features are not supported")
    wav = audio.load(str(path_item))[0]
    if wav.dim() != 2 or wav.size(0) != 1:
        raise ValueError(f"{path_item}: {tuple(wav.shape)} samples; only single-channel audio is supported")
    return path_item.stem, wav


class UtteranceBatch(tuple):
    """(seq [n, 1, L], sizeSeq [n, 1], phone [n, maxSizePhone], sizePhone [n, 1]) on the device, the audio already cut to the
    batch's longest item L: prepare_data passes it on without asking the device for the sizes' maximum."""


class SingleSequenceDataset:
    """The reference's dataset of whole utterances: same attributes (seqOffset, phoneOffsets, maxSize, maxSizePhone) and the same
    four tensors per item.  The audio of all utterances is ONE vector on `device` (the current GPU when there is one); `batches`
    builds a batch with one launch of cpc_gather_utterances."""

    def __init__(self,
                 pathDB,
                 seqNames,
                 phoneLabelsDict,
                 inDim=1,
                 transpose=True,
                 random_offset_amplitude=80,
                 transform=None,
                 device=None):
        if inDim != 1:
            raise ValueError(f"inDim={inDim}: only single-channel audio (inDim=1) is supported, no pre-computed features")
        if transform is not None:
            raise ValueError("transform: the sox augmentation chains of the reference are not supported")
        self.seqNames = deepcopy(seqNames)
        self.pathDB = pathDB
        self.phoneLabelsDict = deepcopy(phoneLabelsDict)
        self.inDim = inDim
        self.transpose = transpose
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.device = torch.device(device)
        self.loadSeqs()
        self.random_offset_amplitude = random_offset_amplitude
        self.transform = transform

    def loadSeqs(self):
        """Decodes every file (in name order), packs the audio into one vector on self.device and the transcriptions into one
        int64 vector, and fills the offset tables."""
        t0 = time.time()
        loaded = sorted((load(Path(self.pathDB) / rel) for _, rel in self.seqNames), key=lambda item: item[0])
        transcripts = [self.phoneLabelsDict[name] for name, _ in loaded]
        sizes = [wav.size(1) for _, wav in loaded]
        n_labels = [len(t) for t in transcripts]

        self.seqOffset = [0]
        self.phoneOffsets = [0]
        for size, n in zip(sizes, n_labels):
            self.seqOffset.append(self.seqOffset[-1] + size)
            self.phoneOffsets.append(self.phoneOffsets[-1] + n)
        self.maxSize = max(sizes, default=0)
        self.maxSizePhone = max(n_labels, default=0)
        self.names = [name for name, _ in loaded]
        self.data = (torch.cat([wav.reshape(-1) for _, wav in loaded]).float() if loaded else torch.zeros(0)).to(self.device)
        self.phoneLabels = torch.tensor([label for t in transcripts for label in t], dtype=torch.long)
        print(f'Loaded {len(self.phoneOffsets)} sequences in {time.time() - t0:.2f} seconds')
        print(f'maxSizeSeq : {self.maxSize}')
        print(f'maxSizePhone : {self.maxSizePhone}')
        print(f"minSizePhone : {min(n_labels, default=float('inf'))}")
        print(f'Total size dataset {sum(sizes) / (16000 * 3600)} hours')

    def _draw_offset(self):
        if self.random_offset_amplitude > 0:
            return random.randint(0, self.random_offset_amplitude)
        return 0

    def __getitem__(self, idx):
        """(audio [1, maxSize] zero padded, its length [1], transcription [maxSizePhone] zero padded, its length [1]); with a
        random offset amplitude the audio starts that many (drawn) samples into the utterance."""
        first, last = self.seqOffset[idx], self.seqOffset[idx + 1]
        p_first, p_last = self.phoneOffsets[idx], self.phoneOffsets[idx + 1]
        first += self._draw_offset()
        outSeq = torch.zeros((self.inDim, self.maxSize), device=self.data.device)
        outSeq[0, :last - first] = self.data[first:last]
        outPhone = torch.zeros(self.maxSizePhone, dtype=torch.long)
        outPhone[:p_last - p_first] = self.phoneLabels[p_first:p_last]
        return outSeq, torch.tensor([last - first], dtype=torch.long), outPhone, torch.tensor([p_last - p_first], dtype=torch.long)

    def __len__(self):
        return len(self.seqOffset) - 1

    def batches(self, batchSize, shuffle):
        """An iterable of UtteranceBatch (len() = batches per epoch; the last one may be smaller).  Every pass draws a new order
        (torch.randperm from the global generator when `shuffle`) and each item's random offset in item order."""
        return _UtteranceLoader(self, batchSize, shuffle)


def gather_utterances(pack, offsets, lengths, roffset, max_len):
    """[n, max_len] zero-padded rows pack[offsets[i] + roffset[i] : offsets[i] + lengths[i]] (int64 device tables)."""
    require_gpu(pack, offsets, lengths, roffset)
    n = offsets.numel()
    out = torch.empty(n, max_len, dtype=torch.float32, device=pack.device)
    check(_lib.load().cpc_gather_utterances(ptr(pack), pack.numel(), ptr(offsets), ptr(lengths), ptr(roffset), ptr(out), n, max_len,
                                            stream_ptr(pack.device)), "gather_utterances")
    return out


class _UtteranceLoader:
    def __init__(self, dataset, batchSize, shuffle):
        if batchSize < 1:
            raise ValueError(f"batchSize={batchSize}")
        self.dataset, self.batchSize, self.shuffle = dataset, batchSize, shuffle

    def __len__(self):
        return (len(self.dataset) + self.batchSize - 1) // self.batchSize

    def __iter__(self):
        ds = self.dataset
        require_gpu(ds.data)
        n = len(ds)
        order = torch.randperm(n).tolist() if self.shuffle else list(range(n))
        dev = ds.data.device
        for at in range(0, n, self.batchSize):
            items = order[at:at + self.batchSize]
            starts = [ds.seqOffset[i] for i in items]
            lengths = [ds.seqOffset[i + 1] - ds.seqOffset[i] for i in items]
            roffsets = [ds._draw_offset() for _ in items]
            phone_sizes = [ds.phoneOffsets[i + 1] - ds.phoneOffsets[i] for i in items]
            sizes = [length - r for length, r in zip(lengths, roffsets)]
            table = torch.tensor([starts, lengths, roffsets, sizes, phone_sizes], dtype=torch.long).to(dev, non_blocking=True)
            phone = torch.zeros(len(items), ds.maxSizePhone, dtype=torch.long)
            for row, i in enumerate(items):
                phone[row, :phone_sizes[row]] = ds.phoneLabels[ds.phoneOffsets[i]:ds.phoneOffsets[i + 1]]
            seq = gather_utterances(ds.data, table[0], table[1], table[2], max(max(sizes), 1))
            yield UtteranceBatch((seq.unsqueeze(1), table[3].view(-1, 1), phone.to(dev, non_blocking=True), table[4].view(-1, 1)))


# --------------------------------------------------------------------------- the head's kernels
class _SeqNormLenFn(torch.autograd.Function):
    """y = (x - m) / sqrt(v + eps) on all frames of x [B, S, H], m and v (unbiased) over the frames < lengths[b]."""

    @staticmethod
    def forward(ctx, x, lengths, eps):
        require_gpu(x, lengths)
        x = f32c(x)
        b, s, h = x.shape
        y = torch.empty_like(x)
        mean = torch.empty(b, h, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        check(_lib.load().cpc_seqnorm_len_forward(ptr(x), ptr(lengths), b, s, h, eps, ptr(y), ptr(mean), ptr(rstd), stream_ptr(x.device)),
              "seqnorm_len_forward")
        ctx.save_for_backward(y, rstd, lengths)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, rstd, lengths = ctx.saved_tensors
        b, s, h = y.shape
        dy = f32c(dy)
        dx = torch.empty_like(y)
        check(_lib.load().cpc_seqnorm_len_backward(ptr(dy), ptr(y), ptr(rstd), ptr(lengths), b, s, h, ptr(dx), stream_ptr(y.device)),
              "seqnorm_len_backward")
        return dx, None, None


def _at(t, elements):
    return ctypes.c_void_p(t.data_ptr() + 4 * elements)


class _ConvHeadFn(torch.autograd.Function):
    """Conv1d(H, C, ks, stride = ks // 2) on channel-last x [B, S, H] -> [B, P, C].  Row j of utterance b is the ks * H contiguous
    floats of x from frame stride * j on, so the product reads x in place with lda = stride * H against the weight repacked to
    [C, ks, H]; the unfolded [B, P, ks * H] matrix never exists.  One product per utterance (its rows end where the utterance
    ends), through cpc_conv_head_forward: cpc_gemm_nt's product with room lent for an ordered sum of its K split (the public
    cpc_gemm_nt adds the parts of a split with atomics).  Backward: db the column sum of dOut, dW from cpc_gemm_tn over the same rows (one slab per utterance, summed in
    utterance order by the column-sum kernel), dx from cpc_conv_head_backward_data."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        require_gpu(x, weight, bias)
        lib = _lib.load()
        x = f32c(x)
        b, s, h = x.shape
        c, hw, ks = weight.shape
        if hw != h:
            raise ValueError(f"CTCphone_criterion: feature width {h} does not match the classifier's {tuple(weight.shape)}")
        if s < ks:
            raise ValueError(f"CTCphone_criterion: {s} frames are fewer than the classifier's kernel size {ks}")
        stride = ks // 2
        p = (s - ks) // stride + 1
        wp = weight.detach().permute(0, 2, 1).contiguous()           # [C, ks, H]
        bvec = f32c(bias.detach())
        out = torch.empty(b, p, c, dtype=torch.float32, device=x.device)
        nb = lib.cpc_conv_head_forward_scratch_bytes(b, s, h, c, ks)
        if nb == 0:
            check(-1, "conv_head_forward shape query")
        buf = scratch(nb, x.device)
        check(lib.cpc_conv_head_forward(ptr(x), ptr(wp), ptr(bvec), ptr(out), b, s, h, c, ks, ptr(buf), buf.numel(), stream_ptr(x.device)),
              "conv_head_forward")
        ctx.save_for_backward(x, wp)
        ctx.geom = (b, s, h, c, ks, p)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        x, wp = ctx.saved_tensors
        b, s, h, c, ks, p = ctx.geom
        stride = ks // 2
        dev = x.device
        st = stream_ptr(dev)
        dout = f32c(dout)
        db = torch.empty(c, dtype=torch.float32, device=dev)
        nb = lib.cpc_probe_xent_backward_scratch_bytes(c)
        check(lib.cpc_probe_head_backward(ptr(dout), b * p, c, None, ptr(db), ptr(scratch(nb, dev)), nb, st), "probe_head_backward")
        width = c * ks * h
        slabs = torch.empty(b, width, dtype=torch.float32, device=dev)
        nt = lib.cpc_gemm_tn_scratch_bytes(c, ks * h, p)
        for i in range(b):
            check(lib.cpc_gemm_tn(_at(dout, i * p * c), c, _at(x, i * s * h), stride * h, _at(slabs, i * width), ks * h, c, ks * h, p,
                                  ptr(scratch(nt, dev)), nt, st), "gemm_tn")
        if b == 1:
            dwp = slabs[0]
        else:
            dwp = torch.empty(width, dtype=torch.float32, device=dev)
            ns = lib.cpc_probe_xent_backward_scratch_bytes(width)
            if ns == 0:
                raise ValueError(f"CTCphone_criterion: a classifier of {c} x {ks} x {h} weights is beyond the column sum's 2^20 columns")
            check(lib.cpc_probe_head_backward(ptr(slabs), b, width, None, ptr(dwp), ptr(scratch(ns, dev)), ns, st), "probe_head_backward")
        dw = dwp.view(c, ks, h).permute(0, 2, 1).contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            check(lib.cpc_conv_head_backward_data(ptr(dout), ptr(wp), b, s, h, c, ks, ptr(dx), st), "conv_head_backward_data")
        return dx, dw, db


class _CTCLossFn(torch.autograd.Function):
    """nn.CTCLoss(blank = K - 1, reduction, zero_infinity=True) of log_softmax(logits [B, T, K]) with input lengths -> loss [1]."""

    @staticmethod
    def forward(ctx, logits, in_lengths, targets, tgt_lengths, reduction):
        require_gpu(logits, in_lengths, targets, tgt_lengths)
        lib = _lib.load()
        logits = f32c(logits)
        b, t, k = logits.shape
        dev = logits.device
        max_l = targets.shape[1]
        nbytes = lib.cpc_ctc_loss_scratch_bytes(b, t, max_l)
        if nbytes == 0:
            check(-1, "ctc_loss shape query")
        want_grad = ctx.needs_input_grad[0]
        nll = torch.empty(b, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        dlogits = torch.empty_like(logits) if want_grad else None
        buf = scratch(nbytes, dev)
        check(lib.cpc_ctc_loss(ptr(logits), b, t, k, ptr(in_lengths), ptr(targets) if max_l else None, max_l, ptr(tgt_lengths),
                               {"sum": 0, "mean": 1}[reduction], ptr(nll), ptr(loss), ptr(dlogits), ptr(buf), buf.numel(),
                               stream_ptr(dev)), "ctc_loss")
        ctx.save_for_backward(dlogits)
        ctx.nll = nll
        return loss

    @staticmethod
    def backward(ctx, dloss):
        (dlogits,) = ctx.saved_tensors
        return dlogits * dloss.reshape(1, 1, 1), None, None, None, None


def ctc_loss(logits, in_lengths, targets, tgt_lengths, reduction='mean'):
    """CTC of logits [B, T, K] (blank = K - 1) with int64 device tables in_lengths [B], targets [B, W], tgt_lengths [B].  The
    padded width W does not matter: it is cut to what the kernel holds, and an utterance whose transcription is longer than T has
    no alignment whatever its input length (loss 0, gradient 0: zero_infinity)."""
    b, t, _k = logits.shape
    in_lengths = in_lengths.to(torch.int64).contiguous()
    tgt_lengths = tgt_lengths.to(torch.int64).contiguous()
    width = min(targets.shape[1], t)
    if width > MAX_TARGET:
        longest = int(tgt_lengths.max().item())
        if longest > MAX_TARGET:
            raise ValueError(f"CTCphone_criterion: a transcription of {longest} labels; cpc_ctc_loss holds up to {MAX_TARGET}")
        width = MAX_TARGET
    if width < targets.shape[1]:
        fits = (tgt_lengths <= width) | (tgt_lengths > targets.shape[1])      # (beyond the given width: the kernel's NaN)
        in_lengths = torch.where(fits, in_lengths, torch.zeros_like(in_lengths))
        tgt_lengths = torch.where(fits, tgt_lengths, torch.zeros_like(tgt_lengths))
    targets = targets[:, :width].to(torch.int64).contiguous()
    return _CTCLossFn.apply(logits, in_lengths, targets, tgt_lengths, reduction)


# --------------------------------------------------------------------------- the criterion
class CTCphone_criterion(torch.nn.Module):

    def __init__(self, dimEncoder, nPhones, LSTM=False, sizeKernel=8,
                 seqNorm=False, dropout=False, reduction='sum'):
        super(CTCphone_criterion, self).__init__()
        if sizeKernel < 2 or sizeKernel % 2:
            raise ValueError(f"CTCphone_criterion: sizeKernel={sizeKernel}; an even size >= 2 is supported (stride = sizeKernel // 2)")
        if reduction not in ('sum', 'mean'):
            raise ValueError(f"CTCphone_criterion: reduction={reduction!r}; 'sum' and 'mean' are supported")
        self.seqNorm = seqNorm
        self.epsilon = 1e-8
        self.dropout = torch.nn.Dropout(
            p=0.5, inplace=False) if dropout else None
        self.conv1 = LSTMPredictor(dimEncoder, dimEncoder,
                                   num_layers=1, batch_first=True)
        self.reduction = reduction
        self.BLANK_LABEL = nPhones
        self.useLSTM = LSTM
        self.downsampling_factor = sizeKernel // 2

        self.PhoneCriterionClassifier = torch.nn.Conv1d(
            dimEncoder, nPhones + 1, sizeKernel, stride=sizeKernel // 2)

    def getPrediction(self, cFeature, featureSize):
        """cFeature [B, S, H], featureSize [B] (frames, integers) -> the classifier's outputs [B, P, nPhones + 1]."""
        require_gpu(cFeature)
        if self.seqNorm:
            sizes = torch.as_tensor(featureSize).to(device=cFeature.device, dtype=torch.int64).view(-1).contiguous()
            if sizes.numel() != cFeature.size(0):
                raise ValueError(f"CTCphone_criterion: {sizes.numel()} sizes for {cFeature.size(0)} utterances")
            cFeature = _SeqNormLenFn.apply(cFeature, sizes, self.epsilon)
        if self.useLSTM:
            cFeature = self.conv1(cFeature)[0]

        if self.dropout is not None:
            cFeature = self.dropout(cFeature.permute(0, 2, 1)).permute(0, 2, 1)

        return _ConvHeadFn.apply(cFeature, self.PhoneCriterionClassifier.weight, self.PhoneCriterionClassifier.bias)

    def forward(self, cFeature, featureSize, label, labelSize):

        predictions = self.getPrediction(cFeature, featureSize)
        dev = predictions.device
        featureSize = torch.as_tensor(featureSize).to(device=dev, dtype=torch.int64).view(-1)
        featureSize = torch.clamp(featureSize // self.downsampling_factor, max=predictions.size(1))
        labelSize = torch.as_tensor(labelSize).to(device=dev, dtype=torch.int64).view(-1)
        label = torch.as_tensor(label).to(device=dev, dtype=torch.int64)
        return ctc_loss(predictions, featureSize, label, labelSize, self.reduction).view(1, -1)

    def align(self, cFeature, featureSize, label, labelSize):
        """The best CTC alignment of every utterance with its transcription (seq_alignment.ctc_forced_align -> AlignResult, on
        the device): getPrediction in eval mode without gradients, the input lengths that forward and perStep use,
        clamp(featureSize // downsampling_factor, max = P)."""
        training = self.training
        self.eval()
        try:
            with torch.no_grad():
                predictions = self.getPrediction(cFeature, featureSize)
        finally:
            self.train(training)
        return self.align_predictions(predictions, featureSize, label, labelSize)

    def align_predictions(self, predictions, featureSize, label, labelSize):
        """align behind getPrediction: the classifier's outputs [B, P, nPhones + 1] and the sizes that getPrediction took."""
        dev = predictions.device
        featureSize = torch.as_tensor(featureSize).to(device=dev, dtype=torch.int64).view(-1)
        featureSize = torch.clamp(featureSize // self.downsampling_factor, max=predictions.size(1))
        labelSize = torch.as_tensor(labelSize).to(device=dev, dtype=torch.int64).view(-1)
        label = torch.as_tensor(label).to(device=dev, dtype=torch.int64)
        return ctc_forced_align(predictions.detach(), featureSize, label, labelSize)


def cut_data(seq, sizeSeq):
    """seq [N, L, ...] cut along dimension 1 to the longest of sizeSeq."""
    return seq[:, :sizeSeq.max()]


def prepare_data(data):
    """A loader's batch -> (audio [n, 1, L], samples [n], transcriptions [n, W], label counts [n]) on the device, the audio cut
    to the batch's longest item.  An UtteranceBatch already is all that."""
    seq, sizeSeq, phone, sizePhone = data
    if isinstance(data, UtteranceBatch):
        return seq, sizeSeq.view(-1), phone, sizePhone.view(-1)
    sizeSeq = sizeSeq.cuda(non_blocking=True).view(-1)
    seq = seq.cuda(non_blocking=True)[:, :, :int(sizeSeq.max())]
    return seq, sizeSeq, phone.cuda(non_blocking=True), sizePhone.cuda(non_blocking=True).view(-1)


def _batch_loss(data, model, criterion, downsampling_factor):
    """The criterion's loss [1, 1] of one batch; the features are detached when the feature maker is frozen."""
    seq, sizeSeq, phone, sizePhone = prepare_data(data)
    c_feature = model(seq, None)[0]
    if not model.optimize:
        c_feature = c_feature.detach()
    return criterion(c_feature, sizeSeq // downsampling_factor, phone, sizePhone)


def train_step(train_loader,
               model,
               criterion,
               optimizer,
               downsampling_factor):
    """One epoch; returns the mean of the batches' losses.  A batch whose loss is not finite takes no step and counts as 0."""
    if model.optimize:
        model.train()
    criterion.train()
    total, n_batches = 0.0, 0
    for data in train_loader:
        optimizer.zero_grad()
        loss = _batch_loss(data, model, criterion, downsampling_factor).mean()
        value = loss.item()
        n_batches += 1
        if not math.isfinite(value):
            print(f"Skipping a batch whose loss is {value}")
            continue
        loss.backward()
        optimizer.step()
        total += value
    return total / n_batches


def val_step(val_loader,
             model,
             criterion,
             downsampling_factor):
    """The mean of the batches' losses in eval mode, without gradients (a loss that is not finite counts as 0)."""
    model.eval()
    criterion.eval()
    total, n_batches = 0.0, 0
    with torch.no_grad():
        for data in val_loader:
            value = _batch_loss(data, model, criterion, downsampling_factor).mean().item()
            total += value if math.isfinite(value) else 0.0
            n_batches += 1
    return total / n_batches


def get_per(data):
    """The reference's get_per on one utterance: (probabilities [T, P], frames, labels, label count, blank) -> PER."""
    pred, size_pred, gt, size_gt, blank_label = data
    l_ = min(int(size_pred) // 4, pred.size(0))          # (the reference's get_per: the default head's stride)
    p_ = pred[:l_].view(l_, -1)
    gt_seq = gt[:int(size_gt)].view(-1).tolist()
    predSeq = beam_search(p_, 20, int(blank_label))[0][1]
    return get_seq_PER(gt_seq, predSeq)


def perStep(val_loader,
            model,
            criterion,
            downsampling_factor):

    model.eval()
    criterion.eval()

    avgPER = 0
    varPER = 0
    nItems = 0
    nTied = 0

    print("Starting the PER computation through beam search")

    for data in val_loader:
        with torch.no_grad():
            seq, sizeSeq, phone, sizePhone = prepare_data(data)
            c_feature, _, _ = model(seq, None)
            sizeSeq = sizeSeq // downsampling_factor
            predictions = torch.nn.functional.softmax(
                criterion.getPrediction(c_feature, sizeSeq), dim=2)
            lengths = torch.clamp(sizeSeq // criterion.downsampling_factor, max=predictions.size(1))
            _, found_sizes, found, _, ties = beam_search_batch(predictions, lengths, 20, criterion.BLANK_LABEL, best_only=True)
            per = get_seq_PER_batch(phone, sizePhone, found[:, 0], found_sizes[:, 0])
            poolData = torch.stack([per, ties.double()]).cpu()
            avgPER += sum([x for x in poolData[0].tolist()])
            varPER += sum([x * x for x in poolData[0].tolist()])
            nItems += poolData.size(1)
            nTied += int((poolData[1] != 0).sum())

    avgPER /= nItems
    varPER /= nItems

    varPER -= avgPER**2
    print(f"Average PER {avgPER}")
    print(f"Standard deviation PER {math.sqrt(max(varPER, 0.0))}")
    print(f"{nTied} of {nItems} utterances met a tie in the beam search")
    return avgPER


# --------------------------------------------------------------------------- forced alignment
SAMPLES_PER_FRAME = 160        # one feature frame (and one written label) per 160 samples
SAMPLE_RATE = 16000


def utterance_alignment(path, labels, confidence, n_samples, blank_label=None, kernel=8, stride=4):
    """One aligned utterance on the host (numpy rows of an AlignResult) -> (frame labels: int64 [n_samples // 160] or None,
    segments: [(label, start_s, end_s, mean log posterior)] one per token).  Both come from seq_alignment's frame map: a blank
    head frame belongs to the preceding token and leading blanks to the first, so the segments tile [0, duration); blank_label
    changes the frame labels only."""
    n_frames = int(n_samples) // SAMPLES_PER_FRAME
    rows = argparse.Namespace(path=path[None], labels=labels[None])
    frames = frame_labels(rows, [n_frames], kernel, stride, blank_label)[0]
    tokens = head_tokens(path)
    segments = []
    if tokens is not None and n_frames > 0:
        by_token = frame_labels(rows, [n_frames], kernel, stride)[0]
        per_frame = tokens[head_frame_of(n_frames, len(tokens), kernel, stride)]
        starts = [0] + [f for f in range(1, n_frames) if per_frame[f] != per_frame[f - 1]]
        for n, f0 in enumerate(starts):
            end = starts[n + 1] * SAMPLES_PER_FRAME / SAMPLE_RATE if n + 1 < len(starts) else int(n_samples) / SAMPLE_RATE
            segments.append((int(by_token[f0]), f0 * SAMPLES_PER_FRAME / SAMPLE_RATE, end, float(confidence[per_frame[f0]])))
    return frames, segments


def write_alignment(frames_file, segments_file, name, frames, segments):
    """One utterance's lines: `name l0 l1 ...` (dataset.parseSeqLabels reads it) and `name phone start_s end_s mean_log_posterior`
    per token."""
    if frames is not None and len(frames):
        frames_file.write(name + " " + " ".join(str(int(v)) for v in frames) + "\n")
    for label, start, end, conf in segments:
        segments_file.write(f"{name} {label} {start:.6f} {end:.6f} {conf:.6f}\n")


def check_align_dir(path):
    """Refuses an output directory that holds anything.  Reads no audio."""
    if os.path.exists(path) and (not os.path.isdir(path) or os.listdir(path)):
        raise ValueError(f"-o {path}: the alignment directory exists and is not empty; give an empty or a new one")


def parse_transcripts(pathPhone):
    """{name: [labels]} of a transcription file `name l0 l1 ...`; unlike dataset.parseSeqLabels a line that holds a name only is
    an empty transcription."""
    out = {}
    with open(pathPhone) as file:
        for line in file:
            data = line.split()
            if data:
                out[data[0]] = [int(x) for x in data[1:]]
    return out


def alignStep(loader, names, model, criterion, downsampling_factor, align_dir, blank_label=None, timings=None):
    """Aligns every utterance of `loader` (batches in the order of `names`) and writes ALIGN_DIR/alignment_frames.txt and
    alignment_segments.txt; returns the counts of alignment_log.json.  One copy to the host per batch.  timings (a dict): seconds
    per stage (audio, model, head, alignment, writing) are added to it, with a device synchronisation behind each stage."""
    model.eval()
    criterion.eval()
    log = dict(utterances=0, aligned=0, no_alignment=[], invalid=[], empty_transcription=[], met_a_tie=0)

    def lap(stage, since):
        if timings is None:
            return since
        torch.cuda.synchronize()
        now = time.perf_counter()
        timings[stage] = timings.get(stage, 0.0) + now - since
        return now

    at = 0
    os.makedirs(align_dir, exist_ok=True)
    with open(os.path.join(align_dir, "alignment_frames.txt"), "w") as frames_file, \
            open(os.path.join(align_dir, "alignment_segments.txt"), "w") as segments_file:
        clock = time.perf_counter()
        for data in loader:
            with torch.no_grad():
                seq, sizeSeq, phone, sizePhone = prepare_data(data)
                clock = lap("audio", clock)
                c_feature = model(seq, None)[0]
                clock = lap("model", clock)
                frames = sizeSeq // downsampling_factor
                predictions = criterion.getPrediction(c_feature, frames)         # (eval mode, no gradients: what align does)
                clock = lap("head", clock)
                res = criterion.align_predictions(predictions, frames, phone, sizePhone)
                t_max, max_l = res.path.shape[1], res.first.shape[1]
                packed = torch.cat([res.path.double(), res.labels.double(), res.first.double(), res.last.double(),
                                    res.confidence.double(), res.status.double().view(-1, 1), res.ties.double().view(-1, 1),
                                    sizeSeq.double().view(-1, 1), sizePhone.double().view(-1, 1)], dim=1).cpu().numpy()
                clock = lap("alignment", clock)
            cuts = [t_max, 2 * t_max, 2 * t_max + max_l, 2 * t_max + 2 * max_l, 2 * t_max + 3 * max_l]
            for row in packed:
                name = names[at]
                at += 1
                path, labels = row[:cuts[0]].astype(np.int64), row[cuts[0]:cuts[1]].astype(np.int64)
                conf = row[cuts[3]:cuts[4]]
                status, tie, n_samples, n_labels = (int(v) for v in row[cuts[4]:cuts[4] + 4])
                log["utterances"] += 1
                if status != 0:
                    log["no_alignment" if status == 1 else "invalid"].append(name)
                    continue
                log["aligned"] += 1
                log["met_a_tie"] += tie
                if n_labels == 0:
                    log["empty_transcription"].append(name)
                write_alignment(frames_file, segments_file, name, *utterance_alignment(path, labels, conf, n_samples, blank_label))
            clock = lap("writing", clock)
    return log


def _with_prefix(state_dict):
    return {f"module.{k}": v for k, v in state_dict.items()}


def _without_prefix(state_dict):
    return {(k[7:] if k.startswith("module.") else k): v for k, v in state_dict.items()}


def load_checkpoint(state_dict, model, criterion):
    """Loads `classifier` and `model` of a checkpoint.pt of `run` (or of the reference's, written under DataParallel): keys with
    or without the `module.` prefix."""
    criterion.load_state_dict(_without_prefix(state_dict['classifier']))
    model.load_state_dict(_without_prefix(state_dict['model']))


def run(train_loader,
        val_loader,
        model,
        criterion,
        optimizer,
        downsampling_factor,
        nEpochs,
        pathCheckpoint):
    """nEpochs of train_step + val_step; checkpoint.pt is rewritten whenever the validation loss improves."""
    print(f"Starting the training for {nEpochs} epochs")
    bestLoss = float('inf')
    for epoch in range(nEpochs):
        print(f"Epoch {epoch} loss train : {train_step(train_loader, model, criterion, optimizer, downsampling_factor)}")
        lossVal = val_step(val_loader, model, criterion, downsampling_factor)
        print(f"Epoch {epoch} loss val : {lossVal}")
        if lossVal >= bestLoss:
            continue
        bestLoss = lossVal
        torch.save(dict(classifier=_with_prefix(criterion.state_dict()), model=_with_prefix(model.state_dict()), bestLoss=bestLoss),
                   pathCheckpoint)


def get_PER_args(args):
    """Completes the arguments of `per` from OUTPUT/args_training.json: data set and extension unless --pathDB is given,
    transcriptions and validation list unless one of them is given, and always the checkpoint and the head's configuration."""
    with open(os.path.join(args.output, "args_training.json")) as file:
        trained = json.load(file)
    if args.pathDB is None:
        args.pathDB, args.file_extension = trained["pathDB"], trained["file_extension"]
    if args.pathVal is None and args.pathPhone is None:
        args.pathPhone, args.pathVal = trained["pathPhone"], trained["pathVal"]
    args.pathCheckpoint, args.no_pretraining = trained["pathCheckpoint"], trained["no_pretraining"]
    for key, default in (("LSTM", False), ("seqNorm", False), ("dropout", False), ("in_dim", 1), ("loss_reduction", "mean")):
        setattr(args, key, trained.get(key, default))
    return args


def parse_args(argv):
    """The reference's two sub-commands with all of their flags and defaults (except --file_extension: .wav)."""
    parser = argparse.ArgumentParser(description="CTC phone recognition on whole utterances: train a head, or score one (per)")
    commands = parser.add_subparsers(dest='command')

    train = commands.add_parser('train', help="train the CTC head (and, unless --freeze, the feature maker)")
    train.add_argument('pathDB', type=str, help="directory of the audio files")
    train.add_argument('pathPhone', type=str, help="text file of the transcriptions: `name l0 l1 ...` per line")
    train.add_argument('pathCheckpoint', type=str, help="CPC checkpoint that makes the features (ID is refused)")
    train.add_argument('--freeze', action='store_true', help="train the head only")
    train.add_argument('--pathTrain', default=None, type=str, help="list of the training utterances (default: all)")
    train.add_argument('--pathVal', default=None, type=str, help="list of the validation utterances (default: a random tenth)")
    train.add_argument('--file_extension', type=str, default=".wav", help=".wav or .flac (.mp3 is refused)")
    train.add_argument('--batchSize', type=int, default=8, help="utterances per batch")
    train.add_argument('--nEpochs', type=int, default=30)
    train.add_argument('--beta1', type=float, default=0.9, help="AdamW beta1")
    train.add_argument('--beta2', type=float, default=0.999, help="AdamW beta2")
    train.add_argument('--epsilon', type=float, default=1e-08, help="AdamW epsilon")
    train.add_argument('--lr', type=float, default=2e-04, help="learning rate of the head (the feature maker gets a tenth)")
    train.add_argument('-o', '--output', type=str, default='out', help="run directory")
    train.add_argument('--debug', action='store_true', help="at most 1000 training and 100 validation utterances")
    train.add_argument('--no_pretraining', action='store_true', help="build the feature maker without loading its weights")
    train.add_argument('--LSTM', action='store_true', help="an LSTM layer in front of the classifier")
    train.add_argument('--seqNorm', action='store_true', help="normalise every utterance's features over its own frames")
    train.add_argument('--kernelSize', type=int, default=8, help="only 8: the reference never passes this flag on")
    train.add_argument('--dropout', action='store_true', help="dropout (0.5) in front of the classifier")
    train.add_argument('--in_dim', type=int, default=1, help="input channels (only 1)")
    train.add_argument('--loss_reduction', type=str, default='mean', choices=['mean', 'sum'])
    train.add_argument('--roffset', type=int, default=0, help="largest random start offset of a training utterance, in samples")
    train.add_argument('-a', '--augments', type=json.loads, nargs='*', default=None, help="refused when given (sox effect chains)")
    train.add_argument('--t_ms', type=int, default=100)

    per = commands.add_parser('per', help="phone error rate of a run directory written by train")
    per.add_argument('output', type=str, help="run directory")
    per.add_argument('--batchSize', type=int, default=8, help="utterances per batch")
    per.add_argument('--debug', action='store_true', help="at most 100 utterances")
    per.add_argument('--pathDB', type=str, default=None, help="another audio directory than the run's")
    per.add_argument('--pathVal', type=str, default=None, help="another list of utterances than the run's")
    per.add_argument('--pathPhone', type=str, default=None, help="other transcriptions than the run's")
    per.add_argument('--file_extension', type=str, default=".wav")
    per.add_argument('--name', type=str, default="0", help="suffix of the log and argument files")

    align = commands.add_parser('align', help="forced alignment of transcriptions with the head of a run directory written by train")
    align.add_argument('output', type=str, help="run directory")
    align.add_argument('-o', '--align_dir', type=str, required=True, help="directory the alignment files are written to (empty or new)")
    align.add_argument('--batchSize', type=int, default=8, help="utterances per batch")
    align.add_argument('--debug', action='store_true', help="at most 100 utterances")
    align.add_argument('--pathDB', type=str, default=None, help="another audio directory than the run's")
    align.add_argument('--pathVal', type=str, default=None, help="another list of utterances than the run's")
    align.add_argument('--pathPhone', type=str, default=None, help="other transcriptions than the run's")
    align.add_argument('--file_extension', type=str, default=".wav")
    align.add_argument('--blank_label', type=int, default=None,
                       help="label written for blank frames (default: a blank frame takes the preceding token's label)")
    align.add_argument('--name', type=str, default="0", help="suffix of the log file")

    args = parser.parse_args(argv)
    if args.command is None:
        parser.error("a command is needed: train, per or align")
    return args


def check_supported(args):
    """Refuses by name what this port does not do.  Reads nothing."""
    extension = args.file_extension
    if extension.lower() == ".mp3":
        raise ValueError("--file_extension .mp3: there is no mp3 decoder in this package; decode the files to .wav or .flac first "
                         "(cpc2_amd.eval.utils.adjust_sample_rate refuses it too)")
    if extension.lower() not in (".wav", ".flac"):
        raise ValueError(f"--file_extension {extension}: only .wav and .flac files can be read")
    if args.pathCheckpoint == 'ID':
        raise ValueError("pathCheckpoint ID: pre-computed .npy features are not supported; give a CPC checkpoint")
    if getattr(args, "in_dim", 1) != 1:
        raise ValueError(f"--in_dim {args.in_dim}: only single-channel audio (--in_dim 1) is supported")
    if getattr(args, "augments", None) is not None:
        raise ValueError("--augments: the sox effect chains of the reference are not supported")
    if getattr(args, "kernelSize", 8) != 8:
        raise ValueError(f"--kernelSize {args.kernelSize}: the reference parses this flag and never hands it to the criterion "
                         "(the head always has kernel size 8); it is refused rather than ignored")


class _Tee(io.TextIOBase):
    """stdout and the log file receive the same text."""

    def __init__(self, *streams):
        self.streams = streams

    def write(self, text):
        for s in self.streams:
            s.write(text)
        return len(text)

    def flush(self):
        for s in self.streams:
            s.flush()


def main(argv):
    args = parse_args(argv)
    random.seed()

    if args.command == 'align':
        check_align_dir(args.align_dir)
    if args.command in ('per', 'align'):
        args = get_PER_args(args)
    check_supported(args)
    if not torch.cuda.is_available():
        raise RuntimeError("cpc2_amd runs only on a GPU (HIP) device and none is available. There is no CPU fallback.")

    if not os.path.isdir(args.output):
        os.mkdir(args.output)

    name = f"_{args.name}" if args.command in ("per", "align") else ""
    pathLogs = os.path.join(args.output, f'logs_{args.command}{name}.txt')
    with open(pathLogs, 'w') as log, contextlib.redirect_stdout(_Tee(sys.stdout, log)):
        return _main(args)


def _split(args, inSeqs):
    """(training utterances, validation utterances): the lists given, else all utterances with a random tenth held out (train)
    or all of them (per)."""
    is_train = args.command == 'train'
    seqTrain = filterSeqs(args.pathTrain, inSeqs) if is_train and args.pathTrain is not None else inSeqs
    if args.pathVal is not None:
        seqVal = filterSeqs(args.pathVal, inSeqs)
    elif is_train:
        random.shuffle(seqTrain)
        cut = int(0.9 * len(seqTrain))
        seqTrain, seqVal = seqTrain[:cut], seqTrain[cut:]
    else:
        seqVal = inSeqs
    if args.debug:
        seqVal = seqVal[:100]
        if is_train:
            print("debug")
            random.shuffle(seqTrain)
            seqTrain = seqTrain[:1000]
    return seqTrain, seqVal


def _main_align(args):
    """`align`: the run is loaded the way `per` loads it; the head's size comes from the checkpoint, so that other
    transcriptions than the run's (a label the head does not know makes that utterance invalid) can be aligned."""
    phoneLabels = parse_transcripts(args.pathPhone)
    inSeqs, _ = findAllSeqs(args.pathDB, extension=args.file_extension, loadCache=False)
    _, seqVal = _split(args, inSeqs)
    pathCheckpoint = os.path.join(args.output, 'checkpoint.pt')
    print(f"Loading data at {pathCheckpoint}")
    state_dict = torch.load(pathCheckpoint, map_location="cpu")
    nPhones = _without_prefix(state_dict['classifier'])['PhoneCriterionClassifier.weight'].shape[0] - 1
    feature_maker, hiddenGar, _ = loadModel([args.pathCheckpoint], loadStateDict=not args.no_pretraining)
    feature_maker.cuda()
    phone_criterion = CTCphone_criterion(hiddenGar, nPhones, args.LSTM, seqNorm=args.seqNorm, dropout=args.dropout,
                                         reduction=args.loss_reduction)
    phone_criterion.cuda()
    load_checkpoint(state_dict, feature_maker, phone_criterion)
    feature_maker.optimize = False
    print(f"Loading the dataset at {args.pathDB}")
    dataset = SingleSequenceDataset(args.pathDB, seqVal, phoneLabels, inDim=args.in_dim, random_offset_amplitude=0)
    t0 = time.time()
    log = alignStep(dataset.batches(args.batchSize, shuffle=False), dataset.names, feature_maker, phone_criterion, 160, args.align_dir,
                    args.blank_label)
    log["seconds"] = time.time() - t0
    log["arguments"] = vars(args)
    with open(os.path.join(args.align_dir, "alignment_log.json"), 'w') as file:
        json.dump(log, file, indent=2)
    print(f"{log['aligned']} of {log['utterances']} utterances aligned ({len(log['no_alignment'])} without a possible alignment, "
          f"{len(log['invalid'])} invalid, {len(log['empty_transcription'])} with an empty transcription, {log['met_a_tie']} met a tie)")
    return log


def _main(args):
    if args.command == 'align':
        return _main_align(args)
    phoneLabels, nPhones = parseSeqLabels(args.pathPhone)
    inSeqs, _ = findAllSeqs(args.pathDB, extension=args.file_extension, loadCache=False)
    seqTrain, seqVal = _split(args, inSeqs)

    downsampling_factor = 160
    feature_maker, hiddenGar, _ = loadModel([args.pathCheckpoint], loadStateDict=not args.no_pretraining)
    feature_maker.cuda()
    phone_criterion = CTCphone_criterion(hiddenGar, nPhones, args.LSTM, seqNorm=args.seqNorm, dropout=args.dropout,
                                         reduction=args.loss_reduction)
    phone_criterion.cuda()

    print(f"Loading the validation dataset at {args.pathDB}")
    datasetVal = SingleSequenceDataset(args.pathDB, seqVal, phoneLabels, inDim=args.in_dim, random_offset_amplitude=0)
    val_loader = datasetVal.batches(args.batchSize, shuffle=True)
    pathCheckpoint = os.path.join(args.output, 'checkpoint.pt')

    if args.command == 'per':
        print(f"Loading data at {pathCheckpoint}")
        state_dict = torch.load(pathCheckpoint, map_location="cpu")
        if 'bestLoss' in state_dict:
            print(f"Best loss : {state_dict['bestLoss']}")
        load_checkpoint(state_dict, feature_maker, phone_criterion)
        feature_maker.optimize = False
        with open(os.path.join(args.output, f"args_validation_{args.name}.json"), 'w') as file:
            json.dump(vars(args), file, indent=2)
        return perStep(val_loader, feature_maker, phone_criterion, downsampling_factor)

    feature_maker.optimize = not args.freeze
    if args.freeze:
        feature_maker.eval()
        for p in feature_maker.parameters():
            p.requires_grad = False
    print(f"Loading the training dataset at {args.pathDB}")
    datasetTrain = SingleSequenceDataset(args.pathDB, seqTrain, phoneLabels, inDim=args.in_dim, random_offset_amplitude=args.roffset)
    train_loader = datasetTrain.batches(args.batchSize, shuffle=True)

    groups = [{'params': list(phone_criterion.parameters())}]
    if not args.freeze:
        print("Optimizing model")
        groups.append({'params': list(feature_maker.parameters()), 'lr': args.lr / 10})
    optimizer = torch.optim.AdamW(groups, lr=args.lr, betas=(args.beta1, args.beta2), eps=args.epsilon)

    with open(os.path.join(args.output, "args_training.json"), 'w') as file:
        json.dump(vars(args), file, indent=2)
    run(train_loader, val_loader, feature_maker, phone_criterion, optimizer, downsampling_factor, args.nEpochs, pathCheckpoint)
    return None


if __name__ == "__main__":
    main(sys.argv[1:])
