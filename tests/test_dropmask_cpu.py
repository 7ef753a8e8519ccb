"""oracle/dropmask.py, the host port of the transformer kernels' dropout masks: statistics of the hash at the index ranges of
a real layer, its constants, and the oracle's handling of the masks.  No GPU: tests/test_transformer_dropout_gpu.py ties the
port to the kernels element for element, which is what makes the statistics below statements about the kernels' masks.

Shape: d_model 256, sizeSeq 116, n = 2 (the criterion's predictors): 2 * 8 * 116 * 116 = 215 296 attention elements and
2 * 116 * 2048 = 475 136 feed-forward elements, p = 0.1, seeds as the module draws them after torch.manual_seed(0..4)."""
import numpy as np
import pytest
import torch

from oracle import cpc_oracle as O
from oracle import dropmask as D
from oracle import synth

P = 0.1
N, SS = 2, 116
N_ATT = N * 8 * SS * SS
N_FFN = N * SS * 2048


def _seed(k):
    torch.manual_seed(k)
    return D.draw_seed()


def _kept(mask):
    return (mask.reshape(-1) != 0).numpy().astype(np.float64)


def _corr(a, b):
    return float(np.corrcoef(a, b)[0, 1])


@pytest.fixture(scope="module", params=range(5))
def masks(request):
    seed = _seed(request.param)
    return seed, _kept(D.attention_mask(seed, N, 1, SS, P)), _kept(D.ffn_mask(seed, N * SS, P))


def test_index_ranges():
    assert N_ATT == 215296 and N_FFN == 475136


def test_keep_rate_is_within_5_sigma_of_0p9(masks):
    """Binomial: sigma = sqrt(p (1 - p) / N) = sqrt(0.09 / N)."""
    _seed_, att, ffn = masks
    for name, kept in (("attention", att), ("ffn", ffn)):
        assert kept.size == (N_ATT if name == "attention" else N_FFN)
        sigma = (0.09 / kept.size) ** 0.5
        assert abs(kept.mean() - 0.9) <= 5 * sigma, (name, kept.mean(), sigma)


def test_neighbouring_elements_are_uncorrelated(masks):
    """|correlation| <= 5 / sqrt(N) (the sample correlation of independent draws has sigma 1 / sqrt(N)) at lag 1 (the next
    key / the next feed-forward unit) and at lag SS (the next query row)."""
    _seed_, att, ffn = masks
    for name, kept in (("attention", att), ("ffn", ffn)):
        for lag in (1, SS):
            c = _corr(kept[:-lag], kept[lag:])
            assert abs(c) <= 5 / (kept.size - lag) ** 0.5, (name, lag, c)


def test_attention_and_ffn_masks_are_uncorrelated_on_common_indices(masks):
    """The two masks of a layer hash the same indices 0 .. under seeds that differ in the low byte only (seed ^ 0xFF)."""
    _seed_, att, ffn = masks
    c = _corr(att, ffn[:N_ATT])
    assert abs(c) <= 5 / N_ATT ** 0.5, c


def test_layers_are_uncorrelated(masks):
    """Layer 1 of a stacked call runs under seed + 0x1000."""
    seed, att, ffn = masks
    s1 = D.layer_seed(seed, 1)
    assert s1 == seed + 0x1000
    c = _corr(att, _kept(D.attention_mask(s1, N, 1, SS, P)))
    assert abs(c) <= 5 / N_ATT ** 0.5, c
    c = _corr(ffn, _kept(D.ffn_mask(s1, N * SS, P)))
    assert abs(c) <= 5 / N_FFN ** 0.5, c


def test_constants():
    assert D.thresh(0.0) == 0
    assert bool((D.attention_mask(_seed(0), 1, 1, 32, 0.0) == 1.0).all())        # thresh 0 keeps everything, scale 1
    assert D.thresh(0.1) == 429496736                                             # float32(0.1) * 2^32, not 0.1 * 2^32 = 429496729
    assert D.thresh(1.0) == 4294967295
    assert D.scale(0.1) == float(np.float32(1) / (np.float32(1) - np.float32(0.1)))
    assert abs(D.scale(0.1) - 1 / 0.9) < 1e-6
    m = D.attention_mask(_seed(1), 1, 1, 32, P)
    assert set(m.unique().tolist()) == {0.0, D.scale(P)}


def test_ffn_seed_differs_from_the_attention_seed():
    seed = _seed(2)
    idx = np.arange(4096, dtype=np.uint64)
    a, b = D.mask_values(seed, idx, P), D.mask_values(seed ^ 0xFF, idx, P)
    assert not np.array_equal(a, b)
    assert np.array_equal(D.ffn_mask(seed, 2, P).numpy().reshape(-1), b)           # ffn_mask IS the hash under seed ^ 0xFF
    assert np.array_equal(D.attention_mask(seed, 1, 1, 8, P).numpy().reshape(-1), a[:8 * 8 * 8])


def _hash32_ints(seed, idx):
    """common.h's hash32 once more in plain Python integers (explicit & 0xFFFFFFFF): the numpy port's wrap-around."""
    m = 0xFFFFFFFF

    def fmix(h):
        h ^= h >> 16
        h = h * 0x85EBCA6B & m
        h ^= h >> 13
        h = h * 0xC2B2AE35 & m
        return h ^ (h >> 16)
    s1 = fmix((seed & m) ^ 0x9E3779B9)
    s2 = fmix(((seed >> 32) + 0x7F4A7C15 + s1) & m)
    return fmix(((((idx & m) ^ s1) * 0x9E3779B1) + ((idx >> 32) ^ s2) * 0x85EBCA77 + s2) & m)


@pytest.mark.parametrize("seed", [0, 0x12345678, 0x1234567800000000, 2 ** 62 - 1, 2 ** 64 - 1])
def test_uint32_arithmetic_wraps_like_the_kernels(seed):
    idx = [0, 1, 2, 115, 116, 2047, 2048, 2 ** 23 + 5, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 7]
    got = D.hash32(seed, np.array(idx, dtype=np.uint64))
    assert got.dtype == np.uint32
    assert [int(v) for v in got] == [_hash32_ints(seed, i) for i in idx]


# ----------------------------------------------------------------------------- the oracle under masks
def test_oracle_with_unit_masks_is_the_eval_mode_oracle_bit_for_bit():
    d, ss, n, s = 64, 32, 2, 80
    p = {k: v.double() for k, v in synth.transformer_params(d, d, ss, 301).items()}
    x = synth.features((n, s, d), 302, relu=True).double()
    ref = O.transformer_layer_forward(x, p, "gAR.0.", size_seq=ss)
    ones = (torch.ones(n * 8 * 3, ss, ss, dtype=torch.float64), torch.ones(n * 3 * ss, 2048, dtype=torch.float64))
    assert torch.equal(O.transformer_layer_forward(x, p, "gAR.0.", size_seq=ss, drop=ones), ref)


def test_oracle_hands_each_block_its_slice_of_the_masks():
    """n = 2 samples of 80 frames in blocks of 32 (3 chunks, the last zero-padded): the layer under the masks of the whole call
    equals block (n_i, c) evaluated alone under the attention masks (n_i * 8 + h) * 3 + c and the FFN rows of that block."""
    d, ss, n, s, chunks = 64, 32, 2, 80, 3
    p = {k: v.double() for k, v in synth.transformer_params(d, d, ss, 303).items()}
    x = synth.features((n, s, d), 304, relu=True).double()
    seed = _seed(3)
    att, ffn = D.layer_masks(seed, n, s, ss, P)
    assert att.shape == (n * 8 * chunks, ss, ss) and ffn.shape == (n * chunks * ss, 2048)
    pre = []
    out = O.transformer_layer_forward(x, p, "gAR.0.", size_seq=ss, drop=(att, ffn), pre_out=pre)
    assert out.shape == (n, s, d) and pre[0].shape == (n * chunks, ss, 2048)
    assert not torch.allclose(out, O.transformer_layer_forward(x, p, "gAR.0.", size_seq=ss))
    xp = torch.cat([x, torch.zeros(n, chunks * ss - s, d, dtype=torch.float64)], dim=1)
    for ni in range(n):
        for c in range(chunks):
            a = torch.stack([att[(ni * 8 + h) * chunks + c] for h in range(8)])
            r0 = (ni * chunks + c) * ss
            blk = O.transformer_layer_forward(xp[ni:ni + 1, c * ss:(c + 1) * ss], p, "gAR.0.", drop=(a, ffn[r0:r0 + ss]))
            keep = min(ss, s - c * ss)
            assert torch.allclose(out[ni, c * ss:c * ss + keep], blk[0, :keep], atol=1e-13, rtol=0)
