"""Window feeder: the step in front of the hot path.

Same names and behaviour as the reference's cpc/dataset.py for the parts the training loop uses --
findAllSeqs (:771-948: every naming convention and the sequence cache), filterSeqs (:963-978), AudioBatchData (:23-408: sequences sorted by
(speaker, name) and concatenated into ONE flat audio vector, speaker / sequence interval tables, chunked
"packs" of at most MAX_SIZE_LOADED samples, getDataLoader with the uniform / sequential / samespeaker /
samesequence / temporalsamespeaker samplers :603-757 and the random window offset :395-403) -- but MI355X-first:
the flat vector lives in HBM (288 GB: the reference's 4e9-sample pack is 16 GB) and a batch is cut out of it
by one gather kernel (cpc_window_gather); the host only produces b int64 offsets per step.  Files are decoded
by the library's own FLAC / WAV readers (cpc2_amd/audio.py).

Signal-quality side files (per-file snr / c50 estimates, dataset.py:69-77,106-120,257-281) are read too and come out as
the third element of a batch.  Frame-level phone labels (parseSeqLabels, dataset.py:97-100,242-245,267-269) replace the
speaker label when given: a pack's labels go to the device once and a batch's [b, sizeWindow // step] labels are gathered there
from the window offsets.

Augmentation (dataset.py:305-321; cpc2_amd/data_augmentation.py): `augmentation` is applied to the past half (`augment_past`),
to the future half with draws of its own (`augment_future`), or once for both (`past_equal_future`).  The loader draws the
numbers of a whole pack's windows on the host before the pack's first step -- window by window, past before future, the "plan"
of the pack (`_AudioLoader.plans`) -- and uploads them with the window offsets; a batch is then built on the device as a
[2, b, 1, W] buffer whose clean half is the gather and whose augmented half is written by the augmentation kernels, and is
yielded as the transposed [b, 2, 1, W] view: sequence[:, 0] and sequence[:, 1] are both contiguous.  `transform` (PeakNorm, the
noise data set's) is applied on the device too.  Labels, phone labels and signal quality are those of the clean windows.
Without augmentation the reference yields past == future (dataset.py:308-321): batches are returned as an
expanded [b, 2, 1, W] view whose two halves alias, which cpcStep(dedup=True) can exploit.
"""
import copy
import os
import random
from pathlib import Path

import torch

from . import _lib, audio
from ._lib import check, ptr, stream_ptr


def _naming_convention(format, extension):
    """(id string of a file name, sort key of a relative path) of one naming convention -- dataset.py:850-865 and :881-937.
    The id is taken from the FILE name, the key from the RELATIVE PATH (directories included), as in the reference."""
    def stem_parts(sep):
        return lambda path: path.replace(extension, '').split(sep)
    if format == "id_spkr_onset_offset":
        return (lambda name: '_'.join(name.split('_')[0:-2]),
                lambda path: ('_'.join(path.split('_')[0:-2]), float(path.split('_')[-2])))
    if format == "id_spkr_onset_offset_spkr_onset_offset":
        return (lambda name: '_'.join(name.split('_')[0:-5]),
                lambda path: ('_'.join(path.split('_')[0:-5]), float(path.split('_')[-5])))
    if format == "spkr-id":
        return (lambda name: '-'.join(name.split('-')[0:2]),
                lambda path: (path.split('-')[0], int(path.split('-')[1])))
    if format == "spkr_id_nb":
        parts = stem_parts('_')
        return (lambda name: '_'.join(name.split('_')[0:-1]), lambda path: (parts(path)[0:-1], int(parts(path)[-1])))
    if format == "spkr-id-nb":
        parts = stem_parts('-')
        return (lambda name: '-'.join(name.split('-')[0:-1]), lambda path: (parts(path)[0:-1], int(parts(path)[-1])))
    if format == "full_seedlings":
        return (lambda name: '_'.join(name.split('_')[0:-2] + [name.split('_')[-1]]),
                lambda path: (path.split('_')[0:-2] + [path.split('_')[-1]], int(path.split('_')[-2])))
    if format == "no_speaker":
        parts = stem_parts('_')
        return (lambda name: 'anonymous', lambda path: (parts(path)[0:-1], int(parts(path)[-1])))
    raise ValueError("%s format unknown" % format)


def findAllSeqs(dirName, no_speaker=False, extension='.flac', loadCache=False, speaker_level=1, format=None,
                cache_path=None):
    """(outSequences [(speaker_index, relative_path)], outSpeakers) -- dataset.py:771-948.

    format=None: speakers are the first `speaker_level` directories, sequences in os.walk order.  With a naming convention
    (`format`, one of cpc_default_config.NAMING_CONVENTIONS): the speaker is the id string cut out of the file name, the list
    is sorted by the convention's (speaker, position) key so that files follow each other in time, and `no_speaker` (or the
    convention 'no_speaker') collapses every id into 'anonymous' with index 0.

    The sequence cache (a torch.save of the two lists; :812-821, :943-947): `loadCache` returns it when it can be read,
    and the listing is saved to it afterwards; `cache_path` defaults to `_seqs_cache.txt` inside dirName.  The cache is
    keyed by nothing -- it does not know the extension, the convention or no_speaker it was made with.  Unlike the
    reference, which saves on EVERY call, a call with neither loadCache nor cache_path reads and writes no file."""
    dirName = str(dirName)
    use_cache = loadCache or cache_path is not None
    if cache_path is None:
        cache_path = str(Path(dirName) / '_seqs_cache.txt')
    if loadCache:
        try:
            outSequences, speakers = torch.load(cache_path)
            print(f'Loaded from cache {cache_path} successfully')
            return outSequences, speakers
        except OSError as err:
            print(f'Ran in an error while loading {cache_path}: {err}')
        print('Could not load cache, rebuilding')
    if dirName[-1] != os.sep:
        dirName += os.sep
    prefixSize = len(dirName)
    id_of, sort_key = _naming_convention(format, extension) if format is not None else (None, None)
    speakersTarget, outSequences = {}, []
    idsTarget, outIds, outSequencesIds = {}, [], []
    for root, _dirs, filenames in os.walk(dirName, followlinks=True):
        filtered_files = [f for f in filenames if f.endswith(extension)]
        if filtered_files:
            speakerStr = os.sep.join(root[prefixSize:].split(os.sep)[:speaker_level])
            speaker = speakersTarget.setdefault(speakerStr, len(speakersTarget))
            for filename in filtered_files:
                full_path = os.path.join(root[prefixSize:], filename)
                outSequences.append((speaker, full_path))
                if format is not None:
                    idStr = 'anonymous' if no_speaker else id_of(filename)
                    if idStr not in idsTarget:
                        idsTarget[idStr] = len(idsTarget)
                        outIds.append(idStr)
                    outSequencesIds.append((idsTarget[idStr], full_path))
    outSpeakers = [None] * len(speakersTarget)
    for key, index in speakersTarget.items():
        outSpeakers[index] = key
    if format is not None:
        outSequences = sorted(outSequencesIds, key=lambda x: sort_key(x[1]))
        if format == "no_speaker" or no_speaker:
            outSequences = [(0, v) for _, v in outSequences]
        outSpeakers = outIds
    if use_cache:
        try:
            torch.save((outSequences, outSpeakers), cache_path)
            print(f'Saved cache file at {cache_path}')
        except (OSError, RuntimeError) as err:          # (torch reports a missing parent directory as RuntimeError)
            print(f'Ran in an error while saving {cache_path}: {err}')
    return outSequences, outSpeakers


def filterSeqs(pathTxt, seqCouples):
    """keep the sequences whose base name is listed in pathTxt -- dataset.py:963-978."""
    with open(pathTxt, 'r') as f:
        wanted = {p.strip() for p in f.readlines() if p.strip()}
    seqCouples = sorted(seqCouples, key=lambda x: os.path.basename(os.path.splitext(x[1])[0]))
    return [x for x in seqCouples if os.path.basename(os.path.splitext(x[1])[0]) in wanted]


def parseSeqLabels(pathLabels):
    """({"step": 160, name: [labels]}, maxLabel + 1) over every line of a label file `name l0 l1 ...` -- dataset.py:951-960."""
    with open(pathLabels, 'r') as f:
        lines = f.readlines()
    output = {"step": 160}          # one label per 160 samples (10 ms at 16 kHz)
    maxPhone = 0
    for line in lines:
        data = line.split()
        output[data[0]] = [int(x) for x in data[1:]]
        maxPhone = max(maxPhone, max(output[data[0]]))
    return output, maxPhone + 1


def shard_for_rank(files, rank, world_size):
    """The contiguous slice of a sequence list one data-parallel rank loads -- cpc/train.py:389-393 (`filter_distributed`):
    files[len * rank // world : len * (rank + 1) // world].  The slices of the world_size ranks partition the list in order,
    sizes differ by at most one, and world_size == 1 returns the list itself.  Applied by the caller to the train, validation
    (and noise) lists alike, after the train / validation split, as the reference does (:396-399)."""
    if not (0 <= rank < world_size):
        raise ValueError(f"shard_for_rank: rank {rank} outside a world of {world_size}")
    start = len(files) * rank // world_size
    end = len(files) * (rank + 1) // world_size
    return files[start:end]


# --------------------------------------------------------------------------- samplers (dataset.py:603-757)
def _uniform_batches(dataSize, sizeWindow, offset, batchSize):
    n = dataSize // sizeWindow - (1 if offset > 0 else 0)
    idx = (offset + sizeWindow * torch.randperm(max(n, 0))).tolist()
    return [idx[i:i + batchSize] for i in range(0, len(idx) - batchSize + 1, batchSize)]      # drop_last=True


def _sequential_batches(dataSize, sizeWindow, offset, batchSize):
    n = (dataSize // sizeWindow) // batchSize - (1 if offset > 0 else 0)
    starts = [x * (dataSize // batchSize) for x in range(batchSize)]
    return [[offset + sizeWindow * i + s for s in starts] for i in range(max(n, 0))]


def _same_interval_batches(intervals, sizeWindow, offset, batchSize):
    """SameSpeakerSampler: every batch comes from one interval (speaker or sequence)."""
    if intervals[0] != 0:
        raise AttributeError("Sampling intervals should start at zero")
    sizes = [(intervals[i + 1] - intervals[i]) // sizeWindow for i in range(len(intervals) - 1)]
    if offset > 0:
        sizes = [max(0, x - 1) for x in sizes]
    batches = []
    for i, val in enumerate(sizes):
        if val <= 0:
            continue
        perm = torch.randperm(val).tolist()
        for s in range(0, val, batchSize):
            batches.append([offset + x * sizeWindow + intervals[i] for x in perm[s:s + batchSize]])
    random.shuffle(batches)
    return batches


def _temporal_same_interval_batches(intervals, sizeWindow, offset, batchSize):
    """TemporalSameSpeakerSampler: a batch is batchSize CONSECUTIVE windows of one interval."""
    if intervals[0] != 0:
        raise AttributeError("Sampling intervals should start at zero")
    sizes = [(intervals[i + 1] - intervals[i]) // (sizeWindow * batchSize) for i in range(len(intervals) - 1)]
    if offset > 0:
        sizes = [max(0, x - 1) for x in sizes]
    if sum(sizes) == 0:
        raise ValueError("No sampling intervals can be found. Try to increase --max_size_loaded or to reduce the batch size.")
    batches = []
    for i, val in enumerate(sizes):
        for x in torch.randperm(val).tolist():
            beg = offset + x * sizeWindow * batchSize + intervals[i]
            batches.append(list(range(beg, beg + sizeWindow * batchSize, sizeWindow)))
    random.shuffle(batches)
    return batches


def remove_artefacts(batches, seqLabel, sizeWindow, carry_shift=False):
    """AudioLoader.__remove_artefacts (dataset.py:486-526) on a list of batches of window offsets: a window that begins in
    sequence i and would run over its end begins at the start of sequence i + 1 instead; in the last sequence it cannot be
    moved and is dropped, and if it was the LAST window of its batch the whole batch is dropped (the reference's flag is
    reset per window, so only the last one decides).  An offset that lies in no sequence is dropped from its batch.
    carry_shift (TemporalSameSpeakerSampler's batches of consecutive windows): the distance a window was moved by is
    added to every later window of the batch, so that they still follow each other.

    The reference walks every boundary for every window; here the sequence is found by bisection -- for the independent
    case for all windows of all batches at once (numpy.searchsorted)."""
    import bisect
    import numpy as np
    n = len(seqLabel)
    if carry_shift:
        out = []
        for batch in batches:
            new_batch, shift, delete = [], 0, False
            for beg in batch:
                beg += shift
                delete = False
                i = bisect.bisect_right(seqLabel, beg)
                if not 1 <= i <= n - 1:
                    continue
                if beg + sizeWindow > seqLabel[i]:
                    if i != n - 1:
                        new_batch.append(seqLabel[i])
                    else:
                        delete = True
                    shift += seqLabel[i] - beg
                else:
                    new_batch.append(beg)
            if not delete:
                out.append(new_batch)
        return out
    if not batches:
        return []
    bounds = np.asarray(seqLabel, dtype=np.int64)
    sizes = np.fromiter((len(b) for b in batches), dtype=np.int64, count=len(batches))
    flat = np.fromiter((o for b in batches for o in b), dtype=np.int64, count=int(sizes.sum()))
    i = np.searchsorted(bounds, flat, side="right")
    inside = (i >= 1) & (i <= n - 1)
    end = bounds[np.clip(i, 0, n - 1)]
    over = inside & (flat + sizeWindow > end)
    stuck = over & (i == n - 1)
    moved = np.where(over, end, flat)
    keep = inside & ~stuck
    stops = np.cumsum(sizes)
    starts = stops - sizes
    out = []
    for lo, hi in zip(starts.tolist(), stops.tolist()):
        if hi > lo and stuck[hi - 1]:
            continue
        out.append(moved[lo:hi][keep[lo:hi]].tolist())
    return out


class PeakNorm(object):
    """dataset.py:433-438: x / (max|x| + 1e-8) of a [C, L] window.  As an AudioBatchData `transform` it runs on the device
    (cpc_augment_peak_norm, or inside the additive-noise kernel for the noise data set)."""

    def __call__(self, x):
        max_val = x.abs().max(dim=1, keepdim=True)[0]
        return x / (max_val + 1e-8)


class AudioBatchData:
    """dataset.py:23-408 (see the module docstring for what is and is not carried over)."""

    def __init__(self, path, sizeWindow, seqNames, phoneLabelsDict, nSpeakers, nProcessLoader=10,
                 MAX_SIZE_LOADED=4000000000, transform=None, augment_past=False, augment_future=False,
                 augmentation=None, keep_temporality=True, past_equal_future=False, signal_quality_path=None,
                 signal_quality_step=1600, signal_quality_mode=None, device=None):
        if transform is not None and not isinstance(transform, PeakNorm):
            raise NotImplementedError("the only window transform on the MI355X feeder path is PeakNorm")
        if augmentation is not None and not all(hasattr(augmentation, name) for name in ("draw_one", "seal", "apply")):
            raise NotImplementedError("augmentation must be a transform of cpc2_amd.data_augmentation (draw_one / seal / apply)")
        self.transform = transform
        self.augment_past = augment_past
        self.augment_future = augment_future
        self.augmentation = augmentation
        self.past_equal_future = past_equal_future
        if self.past_equal_future and not self.augment_past:         # dataset.py:85-87
            raise ValueError("Can only apply the same transformation on past and future sequences,"
                             "when past sequence is augmented. Here --augment_past = False")
        self.MAX_SIZE_LOADED = MAX_SIZE_LOADED
        self.dbPath = Path(path)
        self.sizeWindow = sizeWindow
        self.seqNames = [(s, self.dbPath / x) for s, x in seqNames]
        self.keep_temporality = keep_temporality
        self.speakers = list(range(nSpeakers))
        self.device = torch.device(device) if device is not None else \
            torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.doubleLabels = False
        # dataset.py:97-102: phoneSize samples per label, phoneStep labels per window
        self.phoneSize = 0 if phoneLabelsDict is None else phoneLabelsDict["step"]
        self.phoneStep = 0 if phoneLabelsDict is None else sizeWindow // self.phoneSize
        self.phoneLabelsDict = copy.deepcopy(phoneLabelsDict)
        # signal-quality estimates (dataset.py:69-77,106-120): one .pt per audio file under signal_quality_path (a list of
        # tensors that concatenate along dim 1 to [frames, 2] = (snr, c50), one frame per signal_quality_step samples) and
        # min_max.csv with the normalisation bounds
        self.signal_quality_path = Path(signal_quality_path) if signal_quality_path is not None else None
        self.signal_quality_step = signal_quality_step
        self.signal_quality_size = sizeWindow // signal_quality_step
        self.signal_quality_mode = signal_quality_mode
        self.data_quality = None
        if self.signal_quality_path is not None:
            self._init_min_max_signal_quality()
        self.prepare()
        self.loadNextPack(first=True)
        self.loadNextPack()

    def _init_min_max_signal_quality(self):
        import csv
        file_path = self.signal_quality_path / "min_max.csv"
        if not file_path.is_file():
            raise FileNotFoundError("Can not find file containing min/max values of snr and c50 under: %s" % file_path)
        with open(file_path, "r") as fin:
            reader = csv.reader(fin)
            bounds = dict(zip(next(reader), next(reader)))
        try:
            self.min_snr, self.max_snr = float(bounds["min_snr"]), float(bounds["max_snr"])
            self.min_c50, self.max_c50 = float(bounds["min_c50"]), float(bounds["max_c50"])
        except (KeyError, ValueError):
            raise ValueError("min_max.csv should contain the following keys: min_snr, max_snr, min_c50, max_c50.")

    def resetPhoneLabels(self, newPhoneLabels, step):
        """dataset.py:123-127: new labels (and step) from the next pack on."""
        self.phoneSize = step
        self.phoneStep = self.sizeWindow // self.phoneSize
        self.phoneLabelsDict = copy.deepcopy(newPhoneLabels)
        self.loadNextPack()

    def _quality_file(self, audio_path):
        rel = os.path.relpath(str(audio_path), str(self.dbPath))
        return self.signal_quality_path / (os.path.splitext(rel)[0] + ".pt")       # dataset.py:166-168

    # ---- pack bookkeeping (what dataset.py:147-190 computes, restated on cumulative sizes)
    def prepare(self):
        """New random order of the files (sessions -- runs of equal speaker index -- stay together when keep_temporality) and the
        packs [first file, one past the last) of at most MAX_SIZE_LOADED samples.  The reference's rule, kept because its unit
        tests pin it: a pack is closed by the first file that takes the running size beyond the limit; that file OPENS the next
        pack but is not counted in the next pack's running size, while totSize counts it with the pack it closed."""
        import itertools
        import numpy as np
        if self.keep_temporality:
            sessions = [list(run) for _spk, run in itertools.groupby(self.seqNames, key=lambda item: item[0])]
            random.shuffle(sessions)
            self.seqNames = list(itertools.chain.from_iterable(sessions))
        else:
            random.shuffle(self.seqNames)
        ends = np.cumsum([audio.info(p)[2] for _, p in self.seqNames], dtype=np.int64)      # samples up to and including file i
        n_files = len(ends)
        self.packageIndex, self.totSize = [], 0
        first, counted_from = 0, 0          # the open pack starts at file `first`; its running size counts files >= counted_from
        while True:
            before = int(ends[counted_from - 1]) if counted_from > 0 else 0
            closing = int(np.searchsorted(ends, before + self.MAX_SIZE_LOADED, side="right"))   # first file that exceeds the limit
            if closing >= n_files:
                tail = int(ends[-1]) - before if counted_from < n_files else 0
                if tail > 0:
                    self.packageIndex.append([first, n_files])
                    self.totSize += tail
                break
            self.packageIndex.append([first, closing])
            self.totSize += int(ends[closing]) - before
            first, counted_from = closing, closing + 1
        self.currentPack = -1
        self.nextPack = 0

    def getNPacks(self):
        return len(self.packageIndex)

    def _load_pack(self, pack):
        start, end = self.packageIndex[pack]
        items = []
        for speaker, p in self.seqNames[start:end]:
            wav = audio.load(p)[0].mean(dim=0)              # dataset.py:425: mono mix
            item = (speaker, os.path.splitext(os.path.basename(str(p)))[0], wav)
            if self.signal_quality_path is not None:        # dataset.py:427-430: the audio is cut to whole quality frames
                quality = torch.cat(torch.load(self._quality_file(p)), dim=1).float()
                item = item[:2] + (wav[:quality.shape[0] * self.signal_quality_step], quality)
            items.append(item)
        return items

    def loadNextPack(self, first=False):
        """dataset.py:192-223: make the pack that was read ahead the current one (unless this is the very first call), then read
        the following pack ahead -- cyclically; when the cycle restarts and there is more than one pack, the files are re-shuffled
        and re-packed first."""
        if not first:
            self.currentPack = self.nextPack
            ahead, self.nextData = self.nextData, None
            self.parseNextDataBlock(ahead)
        n_packs = len(self.packageIndex)
        self.nextPack = (self.currentPack + 1) % n_packs
        if n_packs > 1 and self.nextPack == 0:
            self.prepare()
        self.nextData = self._load_pack(self.nextPack)

    def parseNextDataBlock(self, nextData):
        """dataset.py:225-268: the pack's files in (speaker, name) order as ONE flat vector on the device, with the tables of
        where every sequence (seqLabel) and every speaker index up to the last one present (speakerLabel) begins."""
        import numpy as np
        ordered = sorted(nextData, key=lambda item: (item[0], item[1]))
        if self.phoneLabelsDict is not None:
            # dataset.py:242-245: a file's audio is cut to its labels (a file without labels: the reference's KeyError); the pack's
            # labels follow in the same order
            labels = [self.phoneLabelsDict[item[1]] for item in ordered]
            ordered = [item[:2] + (item[2][:len(lab) * self.phoneSize],) + item[3:] for item, lab in zip(ordered, labels)]
            self.phoneLabels = [x for lab in labels for x in lab]
            self.phoneLabelsDevice = torch.tensor(self.phoneLabels, dtype=torch.int64).to(self.device)
            self._phone_range = torch.arange(self.phoneStep, dtype=torch.int64, device=self.device)
        sizes = np.array([item[2].size(0) for item in ordered], dtype=np.int64)
        who = np.array([item[0] for item in ordered], dtype=np.int64)
        valid = set(self.speakers)
        for speaker in who.tolist():
            if speaker not in valid:
                raise ValueError(f'{speaker} invalid speaker')
        self.seqLabel = [0] + np.cumsum(sizes).tolist()
        per_speaker = np.bincount(who, weights=sizes, minlength=int(who.max()) + 1 if len(who) else 1).astype(np.int64)
        self.speakerLabel = [0] + np.cumsum(per_speaker).tolist()
        self.data = torch.cat([item[2] for item in ordered], dim=0).to(self.device)     # resident on the device
        quality = [item[3] for item in ordered if len(item) > 3]
        if quality:                                              # dataset.py:257-265: min-max normalised, third column = mean
            q = torch.cat(quality, dim=0)
            q[:, 0] = (q[:, 0] - self.min_snr) / (self.max_snr - self.min_snr)
            q[:, 1] = (q[:, 1] - self.min_c50) / (self.max_c50 - self.min_c50)
            self.data_quality = torch.cat((q, torch.mean(q, dim=1).view(-1, 1)), dim=1).to(self.device)

    # ---- accessors
    def getPhonem(self, idx):
        """dataset.py:267-269: the labels of the window at sample offset idx (idx need not be a multiple of the step)."""
        idPhone = idx // self.phoneSize
        return self.phoneLabels[idPhone:(idPhone + self.phoneStep)]

    def phonemes_from(self, off_dev):
        """getPhonem of every offset of a device int64 tensor, gathered on the device: [b, phoneStep] int64.  (Window offsets stay
        within data.numel() - sizeWindow, so the last index is at most len(labels) - 1; the clamp only guards the gather.)"""
        first = torch.div(off_dev, self.phoneSize, rounding_mode="floor").unsqueeze(1)
        idx = (first + self._phone_range).clamp_(max=len(self.phoneLabels) - 1)
        return self.phoneLabelsDevice[idx]

    def getSpeakerLabel(self, idx):
        import bisect
        return bisect.bisect_right(self.speakerLabel, idx) - 1

    def getSignalQuality(self, idx):
        """dataset.py:271-281: the window's signal_quality_size estimates of the selected kind."""
        column = {"snr": 0, "c50": 1, "snr_c50": 2}.get(self.signal_quality_mode)
        if column is None:
            raise ValueError("--signal_quality_mode should be in ['snr', 'c50', 'snr_c50'].")
        first = idx // self.signal_quality_step
        return self.data_quality[first:first + self.signal_quality_size, column]

    def __len__(self):
        return self.totSize // self.sizeWindow

    def getNSpeakers(self):
        return len(self.speakers)

    def getNSeqs(self):
        return len(self.seqLabel) - 1

    def getNLoadsPerEpoch(self):
        return len(self.packageIndex)

    def windows(self, offsets):
        """[b, 2, 1, sizeWindow] batch (past and future alias: no augmentation) for int window offsets."""
        b = len(offsets)
        off = torch.tensor(offsets, dtype=torch.int64)
        if self.data.is_cuda:
            return self.windows_from(off.to(self.device))
        out = torch.stack([self.data[o:o + self.sizeWindow] for o in offsets])
        if self.transform is not None:
            out = self.transform(out)
        return out.view(b, 1, self.sizeWindow).unsqueeze(1).expand(b, 2, 1, self.sizeWindow)

    def windows_from(self, off_dev):
        """The same batch from offsets that already are a device int64 tensor (the loader uploads a whole pack's offsets at once)."""
        b = off_dev.numel()
        out = torch.empty(b, 1, self.sizeWindow, dtype=torch.float32, device=self.device)
        self._clean_into(off_dev, out)
        return out.unsqueeze(1).expand(b, 2, 1, self.sizeWindow)

    def _clean_into(self, off_dev, out):
        """The unaugmented windows at `off_dev` (after `transform`) written into the [b, 1, W] buffer `out`."""
        lib = _lib.load()
        if self.transform is not None:
            check(lib.cpc_augment_peak_norm(ptr(self.data), self.data.numel(), ptr(off_dev), ptr(out), off_dev.numel(),
                                            self.sizeWindow, stream_ptr(self.device)), "augment_peak_norm")
        else:
            check(lib.cpc_window_gather(ptr(self.data), self.data.numel(), ptr(off_dev), ptr(out), off_dev.numel(),
                                        self.sizeWindow, stream_ptr(self.device)), "window_gather")
        return out

    def augmented_halves(self):
        """Which halves `augmentation` writes with draws of their own: (past, future) -- dataset.py:308-318."""
        if self.augmentation is None:
            return False, False
        return bool(self.augment_past), bool(self.augment_future) and not self.past_equal_future

    def augmented_from(self, off_dev, plans, lo, hi):
        """The batch of dataset.py:308-321 for the windows at `off_dev`, rows [lo, hi) of the pack's plans (past, future):
        a [2, b, 1, W] buffer seen as [b, 2, 1, W]."""
        from .data_augmentation import FlatWindows
        b, w = off_dev.numel(), self.sizeWindow
        past, future = self.augmented_halves()
        pair = torch.empty(1 if self.past_equal_future else 2, b, 1, w, dtype=torch.float32, device=self.device)
        for half, (on, plan) in enumerate(zip((past, future), plans)):
            if half >= pair.size(0):
                break
            if not on:
                self._clean_into(off_dev, pair[half])
                continue
            src = FlatWindows(self.data, off_dev) if self.transform is None else self._clean_into(off_dev, torch.empty_like(pair[half]))
            self.augmentation.apply(plan, lo, hi, src, pair[half])
        if self.past_equal_future:
            return pair[0].unsqueeze(1).expand(b, 2, 1, w)
        return pair.transpose(0, 1)

    def getBaseSampler(self, type, batchSize, offset, batchSizePerGPU=None):
        n = self.data.numel()
        if type == "samespeaker":
            return _same_interval_batches(self.speakerLabel, self.sizeWindow, offset, batchSize)
        if type == "samesequence":
            return _same_interval_batches(self.seqLabel, self.sizeWindow, offset, batchSize)
        if type == "temporalsamespeaker":
            return _temporal_same_interval_batches(self.speakerLabel, self.sizeWindow, offset, batchSize)
        if type == "sequential":
            return _sequential_batches(n, self.sizeWindow, offset, batchSize)
        if type == "uniform":
            return _uniform_batches(n, self.sizeWindow, offset, batchSize)
        raise ValueError("--samplingType should belong to %s" % ["samespeaker", "samesequence", "temporalsamespeaker",
                                                                "sequential", "uniform"])

    def getDataLoader(self, batchSize, type, randomOffset, numWorkers=0, onLoop=-1, nLoops=-1, remove_artefacts=False,
                      batch_size_per_gpu=None, **unused):
        """Iterable of (sequence [b,2,1,W] on the device, speaker label [b]) over nLoops packs -- dataset.py:366-408.
        remove_artefacts: no window crosses the boundary between two sequences (the module's remove_artefacts, applied to
        every pack's batches before its first step).  batch_size_per_gpu is accepted and, as in the reference (whose
        sampler stores it and never reads it), changes nothing."""
        if onLoop >= 0:
            self.currentPack = onLoop - 1
            self.loadNextPack()
            nLoops = 1 if nLoops <= 0 else nLoops
        elif nLoops <= 0:
            nLoops = len(self.packageIndex)
        return _AudioLoader(self, batchSize, type, randomOffset, nLoops, remove_artefacts)


class _AudioLoader:
    def __init__(self, dataset, batchSize, type, randomOffset, nLoops, remove_artefacts=False):
        self.dataset, self.batchSize, self.type, self.randomOffset, self.nLoops = dataset, batchSize, type, randomOffset, nLoops
        self.remove_artefacts = remove_artefacts

    def _sampler(self):
        d = self.dataset
        if self.randomOffset:                                # dataset.py:395-403
            offset = random.randint(0, d.sizeWindow * self.batchSize) if self.type == "temporalsamespeaker" \
                else random.randint(0, d.sizeWindow // 2)
        else:
            offset = 0
        batches = d.getBaseSampler(self.type, self.batchSize, offset)
        if self.remove_artefacts:                            # dataset.py:478-480
            batches = remove_artefacts(batches, d.seqLabel, d.sizeWindow, carry_shift=self.type == "temporalsamespeaker")
        return batches

    def __len__(self):
        return self.dataset.totSize // (self.dataset.sizeWindow * self.batchSize)

    def _pack_batches(self):
        d = self.dataset
        limit = d.data.numel() - d.sizeWindow
        batches = [[o for o in batch if 0 <= o <= limit] for batch in self._sampler()]
        return [batch for batch in batches if batch]

    def pack_plan(self):
        """The host side of the current pack: its batches of window offsets (the sampler's draws, windows that leave the pack
        dropped) and, with augmentation, the plans of the past and of the future half -- drawn window by window in batch order,
        past before future, as the reference's __getitem__ (dataset.py:308-318) would for these windows in this order.  A pure
        function of the generators' states."""
        d = self.dataset
        batches = self._pack_batches()
        past, future = d.augmented_halves()
        plans = (None, None)
        if past or future:
            import gc
            n = sum(len(batch) for batch in batches)
            entries = ([], [])
            draw, window = d.augmentation.draw_one, d.sizeWindow
            # (the entries are tuples of numbers: nothing for the cyclic collector to find, and its passes over a growing list
            #  -- in a process with torch's objects on the books -- cost four times what the draws do: paused for the loop)
            collecting = gc.isenabled()
            gc.disable()
            try:
                for _ in range(n):
                    if past:
                        entries[0].append(draw(window))
                    if future:
                        entries[1].append(draw(window))
            finally:
                if collecting:
                    gc.enable()
            plans = tuple(d.augmentation.seal(e, d.device) if on else None for e, on in zip(entries, (past, future)))
        return batches, plans

    def offsets(self):
        """(the pack's flat device vector, a batch's window offsets) for every batch of every pack, nothing gathered: how
        AdditiveNoiseAugment takes the noise windows."""
        d = self.dataset
        for loop in range(self.nLoops):
            batches = self._pack_batches()
            data = d.data
            for batch in batches:
                yield data, batch
            if loop + 1 < self.nLoops or len(d.packageIndex) > 1:
                d.loadNextPack()

    def __iter__(self):
        d = self.dataset
        self.plans = []
        augmenting = any(d.augmented_halves())
        if augmenting and not d.data.is_cuda:
            raise RuntimeError("cpc2_amd runs only on a GPU (HIP) device: augmented batches are built by kernels. "
                               "There is no CPU fallback.")
        for loop in range(self.nLoops):
            batches, plans = self.pack_plan()
            if augmenting:
                self.plans.append({"batches": batches, "past": plans[0], "future": plans[1]})
            if d.data.is_cuda and batches:
                # The whole pack's window offsets go to the device in ONE pinned, asynchronous copy and the speaker labels are looked
                # up there (bucketize over the speaker table == dataset.py:254's bisect): a step of the loop then uploads nothing --
                # a pageable `torch.tensor(...).to(device)` per step held the host until the device had caught up, i.e. the loop
                # ran in lock step with the GPU (round 6: host 0.15 ms ahead of the device instead of two steps)
                width = max(len(batch) for batch in batches)
                host = torch.zeros(len(batches), width, dtype=torch.int64).pin_memory()
                for i, batch in enumerate(batches):
                    host[i, :len(batch)] = torch.tensor(batch, dtype=torch.int64)
                offs = host.to(d.device, non_blocking=True)
                table = torch.tensor(d.speakerLabel, dtype=torch.int64).pin_memory().to(d.device, non_blocking=True)
                labels = torch.bucketize(offs, table, right=True) - 1
                row = 0
                for i, batch in enumerate(batches):
                    off_dev, label = offs[i, :len(batch)], labels[i, :len(batch)]
                    if d.phoneSize > 0:                      # dataset.py:298-301: the phone labels replace the speaker's
                        label = d.phonemes_from(off_dev)
                    if augmenting:                           # dataset.py:308-321 (the plan's rows follow the batches)
                        sequence = d.augmented_from(off_dev, plans, row, row + len(batch))
                        row += len(batch)
                    else:
                        sequence = d.windows_from(off_dev)
                    if d.signal_quality_path is not None:    # dataset.py:327-330: a third element per sample
                        yield sequence, label, torch.stack([d.getSignalQuality(o) for o in batch])
                    else:
                        yield sequence, label
            else:
                for batch in batches:
                    if d.phoneSize > 0:
                        label = torch.tensor([d.getPhonem(o) for o in batch], dtype=torch.long, device=d.device)
                    else:
                        label = torch.tensor([d.getSpeakerLabel(o) for o in batch], dtype=torch.long, device=d.device)
                    if d.signal_quality_path is not None:
                        yield d.windows(batch), label, torch.stack([d.getSignalQuality(o) for o in batch])
                    else:
                        yield d.windows(batch), label
            if loop + 1 < self.nLoops or len(d.packageIndex) > 1:
                d.loadNextPack()
