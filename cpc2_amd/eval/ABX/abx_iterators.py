"""ABX item files, features and triplet iterators -- cpc/eval/ABX/abx_iterators.py of the reference, same names, arguments,
random draws and triplet order.

The iterators keep the reference's interface (iterating yields padded group tensors, as loc_dtw expects) and add
`triplets()`, the same traversal with the same `random.sample` calls in the same order, yielding lists of item indices
instead of tensors.  abx_group_computation.get_abx_scores_dtw_on_group plans its batched kernel launches from it.

ABXUnitLoader is the store for quantized units (eval_ABX_clustering): one int32 unit id per frame instead of a one-hot
row, same items, same iterators.
"""
import math
import random

import torch


def normalize_with_singularity(x):
    r"""Normalise along the last dimension and append the singularity column (abx_iterators.py:11-42).  In place on `x`,
    like the reference.  [1, S, H]: the norm gets +1e-12; [S, H]: a zero frame becomes 1/sqrt(H) with a -2e12 border."""
    if len(x.size()) == 3:
        N, S, H = x.size()
        norm_x = (x**2).sum(dim=2, keepdim=True) + 1e-12

        x /= torch.sqrt(norm_x)
        zero_vals = (norm_x == 0).view(N, S)
        x[zero_vals] = 1 / math.sqrt(H)
        border_vect = torch.zeros((N, S, 1), dtype=x.dtype, device=x.device) + 1e-12
        border_vect[zero_vals] = -2 * 1e12
        return torch.cat([x, border_vect], dim=2)

    S, H = x.size()
    norm_x = (x**2).sum(dim=1, keepdim=True)

    x /= torch.sqrt(norm_x)
    zero_vals = (norm_x == 0).view(S)
    x[zero_vals] = 1 / math.sqrt(H)
    border_vect = torch.zeros((S, 1), dtype=x.dtype, device=x.device) + 1e-12
    border_vect[zero_vals] = -2 * 1e12
    return torch.cat([x, border_vect], dim=1)


def load_item_file(path_item_file):
    r"""Parse a .item file (abx_iterators.py:45-92): a header line, then `#file onset offset #phone prev next speaker`
    per line, onsets in seconds.  Returns ({fileID: [[onset, offset, context_id, phone_id, speaker_id], ...]},
    context_match, phone_match, speaker_match); ids are given in first-seen order, the context is 'prev+next'."""
    with open(path_item_file, 'r') as file:
        data = file.readlines()[1:]
    data = [x.replace('\n', '') for x in data]

    out = {}
    phone_match = {}
    speaker_match = {}
    context_match = {}
    for line in data:
        items = line.split()
        if len(items) != 7:
            raise ValueError(f"{path_item_file}: an item line has 7 fields, got {len(items)}: {line!r}")
        fileID = items[0]
        if fileID not in out:
            out[fileID] = []
        onset, offset = float(items[1]), float(items[2])
        context = '+'.join([items[4], items[5]])
        phone = items[3]
        speaker = items[6]
        phone_id = phone_match.setdefault(phone, len(phone_match))
        context_id = context_match.setdefault(context, len(context_match))
        speaker_id = speaker_match.setdefault(speaker, len(speaker_match))
        out[fileID].append([onset, offset, context_id, phone_id, speaker_id])
    return out, context_match, phone_match, speaker_match


def get_features_group(in_data, index_order):
    """Sort the items by the fields `index_order` and nest them into groups of equal values (abx_iterators.py:95-126).
    Returns (sorted item indices, nested groups of (start, end) ranges into that order)."""
    in_index = list(range(len(in_data)))
    in_index.sort(key=lambda x: [in_data[x][i] for i in index_order])
    out_groups = []
    last_values = [in_data[in_index[0]][i] for i in index_order]
    i_s = 0
    curr_group = [[] for i in index_order]
    n_orders = len(index_order) - 1
    tmp = [in_data[i] for i in in_index]

    for index, item in enumerate(tmp):
        for order_index, order in enumerate(index_order):
            if item[order] != last_values[order_index]:
                curr_group[-1].append((i_s, index))
                for i in range(n_orders, order_index, -1):
                    curr_group[i - 1].append(curr_group[i])
                    curr_group[i] = []
                if order_index == 0:
                    out_groups += curr_group[0]
                    curr_group[0] = []
                last_values = [item[i] for i in index_order]
                i_s = index
                break

    if i_s < len(in_data):
        curr_group[-1].append((i_s, len(in_data)))
        for i in range(n_orders, 0, -1):
            curr_group[i - 1].append(curr_group[i])
        out_groups += curr_group[0]

    return in_index, out_groups


class ABXFeatureLoader:
    """All items' features in one [total_frames, D] host tensor (abx_iterators.py:129-257).

    featureMaker(path) gives one file's features ([S, H] or [1, S, H]); with `normalize` they go through
    normalize_with_singularity on the host, once per file.  Item frames: max(0, ceil(step*onset - 0.5)) to
    min(S, floor(step*offset - 0.5)); empty items are skipped.  self.features[i] = [frame offset, size, context_id,
    phone_id, speaker_id]."""

    def __init__(self, path_item_file, seqList, featureMaker, stepFeature, normalize):
        files_data, self.context_match, self.phone_match, self.speaker_match = load_item_file(path_item_file)
        self.seqNorm = True
        self.stepFeature = stepFeature
        self.loadFromFileData(files_data, seqList, featureMaker, normalize)

    def loadFromFileData(self, files_data, seqList, feature_maker, normalize):
        self.features = []
        self.INDEX_CONTEXT = 2
        self.INDEX_PHONE = 3
        self.INDEX_SPEAKER = 4
        data = []
        totSize = 0

        for fileID, file_path in seqList:
            if fileID not in files_data:
                continue
            features = feature_maker(file_path).detach().cpu()
            if normalize:
                features = normalize_with_singularity(features)
            if len(features.size()) > 2:
                features = features.view(features.size(1), features.size(2))

            for phone_start, phone_end, context_id, phone_id, speaker_id in files_data[fileID]:
                index_start = max(0, int(math.ceil(self.stepFeature * phone_start - 0.5)))
                index_end = min(features.size(0), int(math.floor(self.stepFeature * phone_end - 0.5)))
                if index_start >= features.size(0) or index_end <= index_start:
                    continue
                loc_size = index_end - index_start
                self.features.append([totSize, loc_size, context_id, phone_id, speaker_id])
                data.append(features[index_start:index_end])
                totSize += loc_size

        if not data:
            raise ValueError("ABX: no item of the item file has frames in the given sequences "
                             "(check the file IDs, the file extension and --feature_size)")
        self.data = torch.cat(data, dim=0)
        self.feature_dim = self.data.size(1)
        self._frames = {}

    def get_data_device(self):
        return self.data.device

    def cuda(self):
        self.data = self.data.cuda()

    def cpu(self):
        self.data = self.data.cpu()

    def device_frames(self, device, dp):
        """All items' frames on `device` as one [total_frames, dp] fp32 buffer, zero-padded to dp columns, and the
        items' frame offsets and lengths (int32), uploaded once per (device, dp)."""
        key = (str(device), dp)
        if key not in self._frames:
            frames = torch.zeros(self.data.size(0), dp, dtype=torch.float32, device=device)
            frames[:, :self.feature_dim] = self.data.to(device=device, dtype=torch.float32)
            meta = torch.tensor([f[:2] for f in self.features], dtype=torch.int32)
            self._frames[key] = (frames, meta[:, 0].contiguous().to(device), meta[:, 1].contiguous().to(device))
        return self._frames[key]

    def get_max_group_size(self, i_group, i_sub_group):
        id_start, id_end = self.group_index[i_group][i_sub_group]
        return max([self.features[i][1] for i in range(id_start, id_end)])

    def get_ids(self, index):
        context_id, phone_id, speaker_id = self.features[index][2:]
        return context_id, phone_id, speaker_id

    def __getitem__(self, index):
        i_data, out_size, context_id, phone_id, speaker_id = self.features[index]
        return self.data[i_data:(i_data + out_size)], out_size, (context_id, phone_id, speaker_id)

    def __len__(self):
        return len(self.features)

    def get_n_speakers(self):
        return len(self.speaker_match)

    def get_n_context(self):
        return len(self.context_match)

    def get_n_phone(self):
        return len(self.phone_match)

    def get_n_groups(self):
        return len(self.group_index)

    def get_n_sub_group(self, index_sub_group):
        return len(self.group_index[index_sub_group])

    def get_iterator(self, mode, max_size_group, max_x_across=5):
        if mode == 'within':
            return ABXWithinGroupIterator(self, max_size_group)
        if mode == 'across':
            return ABXAcrossGroupIterator(self, max_size_group, max_x_across)
        raise ValueError(f"Invalid mode: {mode}")


class ABXUnitLoader(ABXFeatureLoader):
    """All items' frames as ONE int32 unit id each: `units` [total_frames], where the reference (and ABXFeatureLoader on
    eval_ABX_clustering's feature_function) holds a [total_frames, n_units (+ 1)] one-hot matrix.

    unitMaker(path) gives one file's units, an integer tensor [S] (or [1, S]) with values in [0, n_units).  Items are cut
    with ABXFeatureLoader's onset / offset arithmetic, so self.features is the same table.  The reference-shaped interface
    (__getitem__, the iterators' group_data, iterating an iterator) expands the requested items on demand to the rows the
    reference's loader would hold: the one-hot row as [1, S, n_units] through normalize_with_singularity when `normalize`.
    abx_group_computation.get_abx_scores_dtw_on_group recognises the store and scores it with cpc_abx_dtw_units, without
    ever forming the matrix."""

    def __init__(self, path_item_file, seqList, unitMaker, stepFeature, normalize, n_units):
        if n_units < 1:
            raise ValueError(f"ABXUnitLoader: n_units={n_units} must be at least 1")
        self.n_units = int(n_units)
        self.normalize = bool(normalize)
        super().__init__(path_item_file, seqList, unitMaker, stepFeature, normalize)

    def loadFromFileData(self, files_data, seqList, unit_maker, normalize):
        self.features = []
        self.INDEX_CONTEXT = 2
        self.INDEX_PHONE = 3
        self.INDEX_SPEAKER = 4
        data = []
        totSize = 0

        for fileID, file_path in seqList:
            if fileID not in files_data:
                continue
            units = unit_maker(file_path).detach().cpu()
            if units.is_floating_point() or units.dtype == torch.bool:
                raise TypeError(f"ABXUnitLoader: the unit function must return integer unit ids, got {units.dtype}")
            units = units.reshape(-1)
            if units.numel() and (int(units.min()) < 0 or int(units.max()) >= self.n_units):
                raise ValueError(f"ABXUnitLoader: {file_path} has units outside [0, {self.n_units})")

            for phone_start, phone_end, context_id, phone_id, speaker_id in files_data[fileID]:
                index_start = max(0, int(math.ceil(self.stepFeature * phone_start - 0.5)))
                index_end = min(units.size(0), int(math.floor(self.stepFeature * phone_end - 0.5)))
                if index_start >= units.size(0) or index_end <= index_start:
                    continue
                loc_size = index_end - index_start
                self.features.append([totSize, loc_size, context_id, phone_id, speaker_id])
                data.append(units[index_start:index_end])
                totSize += loc_size

        if not data:
            raise ValueError("ABX: no item of the item file has frames in the given sequences "
                             "(check the file IDs, the file extension and --feature-size)")
        self.units = torch.cat(data, dim=0).to(torch.int32)
        self.feature_dim = self.n_units + (1 if self.normalize else 0)
        self._frames = {}

    def get_data_device(self):
        return self.units.device

    def cuda(self):
        self.units = self.units.cuda()

    def cpu(self):
        self.units = self.units.cpu()

    def expand(self, start, size):
        """Frames start .. start + size - 1 as the rows the reference's loader holds: [size, feature_dim] fp32."""
        u = self.units[start:start + size].long()
        rows = torch.zeros(1, size, self.n_units, dtype=torch.float32, device=u.device)
        rows.scatter_(-1, u.view(1, size, 1), 1)
        if self.normalize:
            rows = normalize_with_singularity(rows)
        return rows.view(size, self.feature_dim)

    def device_frames(self, device, dp):
        raise RuntimeError("ABXUnitLoader holds unit ids, not frames: score it through device_units (cpc_abx_dtw_units)")

    def device_units(self, device):
        """The unit ids on `device` (int32 [total_frames]) and the items' frame offsets and lengths (int32), uploaded
        once per device."""
        key = str(device)
        if key not in self._frames:
            meta = torch.tensor([f[:2] for f in self.features], dtype=torch.int32)
            self._frames[key] = (self.units.to(device).contiguous(), meta[:, 0].contiguous().to(device),
                                 meta[:, 1].contiguous().to(device))
        return self._frames[key]

    def __getitem__(self, index):
        i_data, out_size, context_id, phone_id, speaker_id = self.features[index]
        return self.expand(i_data, out_size), out_size, (context_id, phone_id, speaker_id)


class ABXIterator:
    r"""Base class building ABX's triplets (abx_iterators.py:260-311)."""

    def __init__(self, abxDataset, max_size_group):
        self.max_size_group = max_size_group
        self.dataset = abxDataset
        self.len = 0
        self.index_csp, self.groups_csp = get_features_group(
            abxDataset.features, [abxDataset.INDEX_CONTEXT, abxDataset.INDEX_SPEAKER, abxDataset.INDEX_PHONE])

    def get_group_items(self, i_start, i_end):
        """The dataset indices of one group, sampled down to max_size_group with random.sample as get_group does."""
        to_take = list(range(i_start, i_end))
        if i_end - i_start > self.max_size_group:
            to_take = random.sample(to_take, k=self.max_size_group)
        return [self.index_csp[i] for i in to_take]

    def group_data(self, items):
        """Padded [N, max_size, D] features, sizes and ids of dataset items (the tensors of get_group)."""
        data = [self.dataset[i] for i in items]
        max_size = max(size for _, size, _ in data)
        device = self.dataset.get_data_device()
        out_data = torch.zeros(len(items), max_size, self.dataset.feature_dim, device=device)
        out_size = torch.zeros(len(items), dtype=torch.long, device=device)
        for i, (loc_data, size, _) in enumerate(data):
            out_data[i, :size] = loc_data
            out_size[i] = size
        return out_data, out_size, data[-1][2]

    def get_group(self, i_start, i_end):
        return self.group_data(self.get_group_items(i_start, i_end))

    def triplets(self):
        """Yield (coords, a_items, b_items, x_items) in the reference's order, with its draws."""
        raise NotImplementedError

    def __iter__(self):
        for coords, a, b, x in self.triplets():
            ga = self.group_data(a)
            gb = self.group_data(b)
            gx = ga if x is a else self.group_data(x)
            yield coords, ga[:2], gb[:2], gx[:2]

    def __len__(self):
        return self.len

    def get_board_size(self):
        r"""Get the output dimension of the triplet's space."""
        pass


class ABXWithinGroupIterator(ABXIterator):
    r"""Triplets for the ABX within score (abx_iterators.py:314-360): X is A's own sample; B drawn before A, A redrawn
    for every B."""

    def __init__(self, abxDataset, max_size_group):
        super().__init__(abxDataset, max_size_group)
        self.symmetric = True
        for context_group in self.groups_csp:
            for speaker_group in context_group:
                if len(speaker_group) > 1:
                    for i_start, i_end in speaker_group:
                        if i_end - i_start > 1:
                            self.len += (len(speaker_group) - 1)

    def triplets(self):
        ids = self.dataset.get_ids
        for i_c, context_group in enumerate(self.groups_csp):
            for i_s, speaker_group in enumerate(context_group):
                n_phones = len(speaker_group)
                if n_phones == 1:
                    continue
                for i_a in range(n_phones):
                    i_start_a, i_end_a = speaker_group[i_a]
                    if i_end_a - i_start_a == 1:
                        continue
                    for i_b in range(n_phones):
                        if i_b == i_a:
                            continue
                        i_start_b, i_end_b = speaker_group[i_b]
                        b = self.get_group_items(i_start_b, i_end_b)
                        a = self.get_group_items(i_start_a, i_end_a)
                        c_a, p_a, s_a = ids(a[-1])
                        p_b = ids(b[-1])[1]
                        yield (s_a, p_a, p_b, c_a), a, b, a

    def get_board_size(self):
        return (self.dataset.get_n_speakers(), self.dataset.get_n_phone(), self.dataset.get_n_phone(),
                self.dataset.get_n_context())


class ABXAcrossGroupIterator(ABXIterator):
    r"""Triplets for the ABX across score (abx_iterators.py:363-448): up to max_x_across other speakers of the same
    (context, phone) as X; draws in the order A, B, X per triplet."""

    def __init__(self, abxDataset, max_size_group, max_x_across):
        super().__init__(abxDataset, max_size_group)
        self.symmetric = False
        self.get_speakers_from_cp = {}
        self.max_x = max_x_across

        for context_group in self.groups_csp:
            for speaker_group in context_group:
                for i_start, i_end in speaker_group:
                    c_id, p_id, s_id = self.dataset.get_ids(self.index_csp[i_start])
                    self.get_speakers_from_cp.setdefault(c_id, {}).setdefault(p_id, {})[s_id] = (i_start, i_end)

        for context_group in self.groups_csp:
            for speaker_group in context_group:
                if len(speaker_group) > 1:
                    for i_start, i_end in speaker_group:
                        c_id, p_id, s_id = self.dataset.get_ids(self.index_csp[i_start])
                        self.len += (len(speaker_group) - 1) * (min(self.max_x,
                                                                    len(self.get_speakers_from_cp[c_id][p_id]) - 1))

    def get_other_speakers_in_group(self, i_start_group):
        c_id, p_id, s_id = self.dataset.get_ids(self.index_csp[i_start_group])
        return [v for k, v in self.get_speakers_from_cp[c_id][p_id].items() if k != s_id]

    def get_abx_triplet_items(self, i_a, i_b, i_x):
        ids = self.dataset.get_ids
        a = self.get_group_items(*i_a)
        b = self.get_group_items(*i_b)
        x = self.get_group_items(*i_x)
        c_a, p_a, s_a = ids(a[-1])
        return (s_a, p_a, ids(b[-1])[1], c_a, ids(x[-1])[2]), a, b, x

    def get_abx_triplet(self, i_a, i_b, i_x):
        coords, a, b, x = self.get_abx_triplet_items(i_a, i_b, i_x)
        return coords, self.group_data(a)[:2], self.group_data(b)[:2], self.group_data(x)[:2]

    def triplets(self):
        for i_c, context_group in enumerate(self.groups_csp):
            for i_s, speaker_group in enumerate(context_group):
                n_phones = len(speaker_group)
                if n_phones == 1:
                    continue
                for i_a in range(n_phones):
                    i_start_a, i_end_a = speaker_group[i_a]
                    ref = self.get_other_speakers_in_group(i_start_a)
                    if len(ref) > self.max_x:
                        speakers_a = random.sample(ref, k=self.max_x)
                    else:
                        speakers_a = ref
                    for i_start_x, i_end_x in speakers_a:
                        for i_b in range(n_phones):
                            if i_b == i_a:
                                continue
                            yield self.get_abx_triplet_items((i_start_a, i_end_a), speaker_group[i_b],
                                                             (i_start_x, i_end_x))

    def get_board_size(self):
        return (self.dataset.get_n_speakers(), self.dataset.get_n_phone(), self.dataset.get_n_phone(),
                self.dataset.get_n_context(), self.dataset.get_n_speakers())
