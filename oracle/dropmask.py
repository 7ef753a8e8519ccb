"""Host port of the transformer kernels' dropout masks (oracle, test infrastructure only).

The kernels do not draw their masks from a random stream: the multiplier of an element is a pure 32-bit hash of
(seed, element index) -- drop_mul in cpc2_amd/csrc/common.h -- recomputed wherever it is needed (attention forward and
backward, the feed-forward activation's GEMM epilogue).  The seed comes from torch's CPU generator
(cpc2_amd/transformers.py, TransformerLayer.forward), so a test can rebuild every mask bit for bit:

    attention   [n * 8 * chunks, SS, SS]   element ((n_i * 8 + h) * chunks + c) * SS * SS + i * SS + j     under the layer's seed
    FFN         [rows, 2048]               element row * 2048 + col, rows = n * chunks * SS (padded rows)   under seed ^ 0xFF
    layer l of a stacked call              seed + 0x1000 * l

Plain numpy in uint32 arithmetic (wrap-around is the point).  Never imported by the product package (cpc2_amd/).
"""
import numpy as np
import torch

N_HEADS = 8         # TR_HEADS
D_FF = 2048         # TR_DFF
_M32 = 0xFFFFFFFF
_M64 = 0xFFFFFFFFFFFFFFFF


def fmix32(h):
    """murmur3's 32-bit finaliser (common.h: fmix32) on a uint32 array."""
    h = np.asarray(h, dtype=np.uint32).copy()
    with np.errstate(over="ignore"):
        h ^= h >> np.uint32(16)
        h *= np.uint32(0x85EBCA6B)
        h ^= h >> np.uint32(13)
        h *= np.uint32(0xC2B2AE35)
        h ^= h >> np.uint32(16)
    return h


def hash32(seed, idx):
    """common.h: hash32(seed, idx) -- seed a Python int (64 bits), idx an integer array of element indices (64 bits)."""
    seed = int(seed) & _M64
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        s1 = fmix32(np.array([(seed & _M32) ^ 0x9E3779B9], dtype=np.uint32))
        s2 = fmix32(np.array([seed >> 32], dtype=np.uint32) + np.uint32(0x7F4A7C15) + s1)
        lo = (idx & np.uint64(_M32)).astype(np.uint32)
        hi = (idx >> np.uint64(32)).astype(np.uint32)
        return fmix32((lo ^ s1) * np.uint32(0x9E3779B1) + (hi ^ s2) * np.uint32(0x85EBCA77) + s2)


def thresh(p):
    """transformer.hip: drop_thresh -- the float32 value of p times 2^32, capped (0.1 -> 429496736, not 429496729)."""
    p32 = float(np.float32(p))
    return 0 if p32 <= 0.0 else int(min(4294967295.0, p32 * 4294967296.0))


def scale(p):
    """1 / (1 - p) in float32, as a Python float."""
    p32 = np.float32(p)
    return float(np.float32(1) / (np.float32(1) - p32)) if p32 > 0 else 1.0


def mask_values(seed, idx, p):
    """drop_mul for every element index of `idx`: float64 array of `scale(p)` (kept) or 0 (dropped)."""
    th = thresh(p)
    idx = np.asarray(idx)
    if th == 0:
        return np.full(idx.shape, scale(p))
    return np.where(hash32(seed, idx) >= np.uint32(th), scale(p), 0.0)


def attention_mask(seed, n, chunks, size_seq, p):
    """[n * 8 * chunks, SS, SS] float64 tensor: the multiplier of the softmax output of (sample n_i, head h, chunk c) at
    (query i, key j), in the kernels' order (n_i * 8 + h) * chunks + c."""
    count = n * N_HEADS * chunks * size_seq * size_seq
    m = mask_values(seed, np.arange(count, dtype=np.uint64), p)
    return torch.from_numpy(m).view(n * N_HEADS * chunks, size_seq, size_seq)


def ffn_mask(seed, rows, p):
    """[rows, 2048] float64 tensor: the multiplier of relu(lin1) -- hashed under seed ^ 0xFF; rows counts the padded rows."""
    m = mask_values((int(seed) & _M64) ^ 0xFF, np.arange(rows * D_FF, dtype=np.uint64), p)
    return torch.from_numpy(m).view(rows, D_FF)


def layer_seed(seed, layer):
    """Seed of layer `layer` of a stacked call (transformer.hip: seed + 0x1000 * l, 64-bit wrap-around)."""
    return (int(seed) + 0x1000 * int(layer)) & _M64


def layer_masks(seed, n, s, size_seq, p, layer=0):
    """(attention mask, FFN mask) of one layer applied to an input [n, s, .] attended in blocks of size_seq frames."""
    chunks = -(-s // size_seq)
    ls = layer_seed(seed, layer)
    return attention_mask(ls, n, chunks, size_seq, p), ffn_mask(ls, n * chunks * size_seq, p)


def draw_seed():
    """The draw TransformerLayer.forward makes from torch's CPU generator in training mode: call after the same
    torch.manual_seed to obtain the seed the module will use (and once more for every further training-mode call)."""
    return int(torch.randint(0, 2 ** 62, (1,)).item())
