"""collapseLabelChain of the reference's cpc/criterion/seq_alignment.py (:62-84) on the device (cpc_probe_collapse)."""
import torch

from . import _lib
from ._lib import check, ptr, require_gpu, stream_ptr


def collapse_padded(inputLabels):
    """[N, T] frame labels -> (targets int64 [N, T], sizes int64 [N]): consecutive repeats removed, zero padded to T.  Nothing
    comes to the host (the CTC kernel takes the padded width as it is)."""
    require_gpu(inputLabels)
    labels = inputLabels.to(torch.int64).contiguous()
    n, t = labels.shape
    out = torch.empty(n, t, dtype=torch.int64, device=labels.device)
    sizes = torch.empty(n, dtype=torch.int64, device=labels.device)
    check(_lib.load().cpc_probe_collapse(ptr(labels), n, t, ptr(out), t, ptr(sizes), stream_ptr(labels.device)), "probe_collapse")
    return out, sizes


def collapseLabelChain(inputLabels):
    """(paddedOutput int64 [N, maxS], outSizes int64 [N]) with maxS the batch's largest collapsed length, as the reference
    returns it (one small copy to the host for maxS)."""
    out, sizes = collapse_padded(inputLabels)
    maxSize = int(sizes.max().item())
    return out[:, :maxSize].contiguous(), sizes
