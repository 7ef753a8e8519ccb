"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, reached through the C ABI of
libcpc2_hip.so, against (a) golden vectors produced by the reference implementation and (b) the
CPU oracle (float64 where a tighter check of the fp32 kernels is useful).

Tolerances: fp32 kernels vs fp64 oracle -> 2e-5 relative to the tensor's scale unless noted;
the InfoNCE LOSS must be within 1e-3 relative (north_star), negative indices bit-exact."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cpc2_amd
from cpc2_amd import _lib
from cpc2_amd.train import FlatAdam, buildOptimizer, cpcStep
from oracle import cpc_oracle as O
from oracle import synth
from oracle.mt19937 import MT19937, negative_indices

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def t(a):
    return torch.from_numpy(np.asarray(a))


def rel_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def assert_close(got, ref, tol, what="", rtol=None):
    """max-norm check |got - ref|_inf <= tol * |ref|_inf AND, element by element, |got - ref| <= atol + rtol * |ref| with
    atol = tol * |ref|_inf (rounding noise scales with the largest terms of a sum) and rtol = 64 * tol by default: a
    small element may be off by the noise floor, but not arbitrarily."""
    e = rel_err(got, ref)
    assert e <= tol, f"{what}: rel err {e:.3e} > {tol:.1e}"
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    atol = tol * float(r.abs().max()) + 1e-30
    rt = 64 * tol if rtol is None else rtol
    bad = (g - r).abs() > atol + rt * r.abs()
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements outside atol {atol:.2e} + {rt:.1e} |ref|"


def load_encoder(hidden, params):
    enc = cpc2_amd.CPCEncoder(hidden)
    enc.load_state_dict({k[len("gEncoder."):]: v for k, v in params.items()})
    return enc.to(DEV)


def to64(p):
    return {k: v.double() for k, v in p.items()}


# ----------------------------------------------------------------------------- GEMMs
# (65536, 128, 1024) and (32768 + 77, 256, 1056): the software-pipelined 256 x 128 kernel (whole rounds of 256 workgroups),
# the second with a ragged last row tile and an odd number of K steps
@pytest.mark.parametrize("m,n,k", [(128, 128, 32), (300, 200, 72), (1, 5, 3), (1026, 256, 2048), (257, 770, 24),
                                   (65536, 128, 1024), (32768 + 77, 256, 1056)])
def test_gemm_nt(m, n, k):
    lib = _lib.load()
    g = torch.Generator().manual_seed(m * 7 + n)
    a, b, bias = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g), torch.randn(n, generator=g)
    ad, bd, biasd = a.to(DEV), b.to(DEV), bias.to(DEV)
    c = torch.full((m, n), float("nan"), device=DEV)
    _lib.check(lib.cpc_gemm_nt(_lib.ptr(ad), k, _lib.ptr(bd), k, _lib.ptr(c), n, _lib.ptr(biasd), m, n, k, _lib.stream_ptr(c.device)))
    ref = a.double() @ b.double().t() + bias.double()
    assert_close(c, ref, 2e-6 * max(1, k ** 0.5), "gemm_nt")


def test_gemm_nt_overlapping_rows_is_a_strided_conv():
    """A rows with lda < K: the implicit-GEMM form of Conv1d over a channel-last signal."""
    lib = _lib.load()
    c_in, c_out, k, s, length = 32, 64, 8, 4, 400
    g = torch.Generator().manual_seed(3)
    x = torch.randn(length, c_in, generator=g)                       # channel-last
    w = torch.randn(c_out, c_in, k, generator=g)
    rows = (length - k) // s + 1
    wr = w.permute(0, 2, 1).reshape(c_out, k * c_in).contiguous()
    out = torch.empty(rows, c_out, device=DEV)
    xd, wd = x.to(DEV), wr.to(DEV)
    _lib.check(lib.cpc_gemm_nt(_lib.ptr(xd), s * c_in, _lib.ptr(wd), k * c_in, _lib.ptr(out), c_out, None, rows, c_out, k * c_in,
                               _lib.stream_ptr(out.device)))
    ref = torch.nn.functional.conv1d(x.t().unsqueeze(0).double(), w.double(), stride=s)[0].t()
    assert_close(out, ref, 1e-5, "strided-A gemm")


@pytest.mark.parametrize("m,n,r", [(128, 128, 64), (256, 2048, 5000), (96, 24, 333), (3, 5, 7), (768, 256, 2064)])
def test_gemm_tn(m, n, r):
    lib = _lib.load()
    g = torch.Generator().manual_seed(m + n + r)
    a, b = torch.randn(r, m, generator=g), torch.randn(r, n, generator=g)
    ad, bd = a.to(DEV), b.to(DEV)
    c = torch.full((m, n), float("nan"), device=DEV)
    nbytes = lib.cpc_gemm_tn_scratch_bytes(m, n, r)
    sc = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    _lib.check(lib.cpc_gemm_tn(_lib.ptr(ad), m, _lib.ptr(bd), n, _lib.ptr(c), n, m, n, r, _lib.ptr(sc), nbytes, _lib.stream_ptr(c.device)))
    ref = a.double().t() @ b.double()
    assert_close(c, ref, 2e-6 * max(1, r ** 0.5), "gemm_tn")


def _gemm_rel_err(kind, a, b, mode):
    """max and rms of |C - C64| / (|A| . |B|) with the GEMM family `mode` (0 bf16x6 split, 1 f32 MFMA)."""
    lib = _lib.load()
    prev = lib.cpc_gemm_set_mode(mode)
    try:
        ad, bd = a.to(DEV), b.to(DEV)
        if kind == "nt":
            m, k = a.shape
            n = b.shape[0]
            c = torch.empty(m, n, device=DEV)
            _lib.check(lib.cpc_gemm_nt(_lib.ptr(ad), k, _lib.ptr(bd), k, _lib.ptr(c), n, None, m, n, k, _lib.stream_ptr(c.device)))
            ref, mag = a.double() @ b.double().t(), a.double().abs() @ b.double().abs().t()
        else:
            r, m = a.shape
            n = b.shape[1]
            c = torch.empty(m, n, device=DEV)
            nbytes = lib.cpc_gemm_tn_scratch_bytes(m, n, r)
            sc = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
            _lib.check(lib.cpc_gemm_tn(_lib.ptr(ad), m, _lib.ptr(bd), n, _lib.ptr(c), n, m, n, r, _lib.ptr(sc), nbytes, _lib.stream_ptr(c.device)))
            ref, mag = a.double().t() @ b.double(), a.double().abs().t() @ b.double().abs()
    finally:
        lib.cpc_gemm_set_mode(prev)
    e = (c.cpu().double() - ref).abs() / mag.clamp_min(1e-300)
    return float(e.max()), float(e.pow(2).mean().sqrt())


@pytest.mark.parametrize("kind,shape,data", [("nt", (2048, 256, 2048), "randn"), ("nt", (2048, 256, 512), "relu"),
                                             ("nt", (1024, 768, 256), "wide"), ("tn", (8192, 256, 1024), "randn"),
                                             ("tn", (4000, 256, 512), "tiny")])
def test_gemm_split_accuracy(kind, shape, data):
    """The default GEMMs run on the bf16 pipe from an exact three-term split of the f32 operands; their error
    against an fp64 product must be that of an f32 GEMM: no worse than the f32-MFMA kernels' (mode 1) on the
    same data, and within a few f32 roundings of sum |a||b|."""
    g = torch.Generator().manual_seed(sum(shape))
    if kind == "nt":
        m, n, k = shape
        a, b = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g) / k ** 0.5
    else:
        r, m, n = shape
        a, b = torch.randn(r, m, generator=g), torch.randn(r, n, generator=g)
    if data == "relu":
        a = a.clamp_min(0)
    if data == "wide":        # magnitudes over 2^-20 .. 2^20 within one row: residual terms at every exponent
        a = a * torch.exp2(torch.randint(-20, 21, a.shape, generator=g).float())
    if data == "tiny":        # gradient-sized operands
        a, b = a * 1e-9, b * 1e-7
    split_max, split_rms = _gemm_rel_err(kind, a, b, 0)
    f32_max, f32_rms = _gemm_rel_err(kind, a, b, 1)
    assert split_rms <= 1.25 * f32_rms + 1e-10, (split_rms, f32_rms)
    assert split_max <= 1.5 * f32_max + 1e-9, (split_max, f32_max)
    assert split_max <= 16 * 2.0 ** -24


SEQ_F32_RMS = 3.5e-8      # rms error / sum |a||b| of a dot product accumulated term by term in f32 (2^-25 = 3.0e-8)


def _to_planes(lib, x, stride_log2=0):
    """x[rows][cols] (f32, device) -> its three bf16 planes in 16-channel chunks (cpc_split_planes); rows padded to the stride."""
    rows, cols = x.shape
    s = 1 << stride_log2
    assert rows % s == 0
    rts = rows // s
    plane = (cols // 16) * s * rts * 16
    out = torch.zeros(3 * plane, dtype=torch.int16, device=x.device)
    _lib.check(lib.cpc_split_planes(_lib.ptr(x), cols, rows, cols, _lib.ptr(out), plane, stride_log2, rts, _lib.stream_ptr(x.device)))
    return out, plane, rts


@pytest.mark.parametrize("taps,stride,n_win,frames,cols,data", [(8, 4, 5, 130, 256, "relu"), (4, 2, 3, 257, 512, "randn"),
                                                               (1, 1, 1, 1000, 256, "wide"), (8, 4, 40, 128, 256, "tiny")])
def test_plane_fed_gemm_nt_accuracy(taps, stride, n_win, frames, cols, data):
    """cpc_gemm_nt_planes (operands stored as the three bf16 terms of every f32, six MFMA products): a strided Conv1d over a
    channel-last signal as ONE product.  Its error against fp64 must be an f32 GEMM's.  Two f32 GEMMs are the yardstick:
    the f32-MFMA kernel (cpc_gemm_nt, mode 1) on the same overlapping rows, and torch's f32 matmul of the unfolded rows.
    The plane-fed kernel adds K / 16 x 6 MFMA results into ONE f32 accumulator per element: six roundings of the running sum
    per 16 terms where an f32-MFMA chain has four, so its noise is 1.2-1.8 x that chain's and equal to a sequential f32 FMA
    sum's (2-3e-8 of sum |a||b| rms whatever K; torch's matmul measures 2.8e-8 at M >= 1024).  Both yardsticks split K
    over workgroups when M is small and then come out below that -- hence the absolute allowance SEQ_F32_RMS."""
    lib = _lib.load()
    H = 256
    g = torch.Generator().manual_seed(taps * 1000 + frames)
    R = stride * (frames + 2) if taps > 1 else frames             # signal rows per window
    rows = n_win * R + 2 * stride
    y = torch.randn(rows, H, generator=g)
    if data == "relu":
        y = y.clamp_min(0)
    if data == "wide":
        y = y * torch.exp2(torch.randint(-20, 21, y.shape, generator=g).float())
    w = torch.randn(cols, taps * H, generator=g) / (taps * H) ** 0.5
    if data == "tiny":
        y, w = y * 1e-9, w * 1e-7
    bias = torch.randn(cols, generator=g) * float(y.abs().max() * w.abs().max())
    yd, wd, bd = y.to(DEV), w.to(DEV), bias.to(DEV)
    sl = stride.bit_length() - 1
    K = taps * H
    yp, ya, rts = _to_planes(lib, yd, sl)
    order = [(jj >> 1) + (jj & 1) * stride for jj in range(taps)] if taps > 1 else [0]
    wk = wd.view(cols, taps, H // 16, 16)[:, order].permute(0, 2, 1, 3).reshape(cols, K).contiguous()
    wp, wa, _ = _to_planes(lib, wk)
    # the planes add up to the operand EXACTLY (three bf16 terms hold 24 bits) unless a term falls under the bf16 range
    rec = sum(yp[i * ya:(i + 1) * ya].view(torch.bfloat16).double() for i in range(3)).view(H // 16, stride, rts, 16)
    rec = rec.permute(2, 1, 0, 3).reshape(rows, H)
    if data != "tiny":
        assert torch.equal(rec.cpu(), y.double())
    M = n_win * frames
    c = torch.empty(M, cols, device=DEV)
    _lib.check(lib.cpc_gemm_nt_planes(_lib.ptr(yp), ya, taps.bit_length() - 1, sl, rts, frames, R // stride, _lib.ptr(wp), wa,
                                      _lib.ptr(c), cols, _lib.ptr(bd), M, cols, K, _lib.stream_ptr(c.device)))
    # the same product by the f32-MFMA kernel: virtual rows of stride * H floats, window n starts at row n * R / stride
    virt = n_win * (R // stride)
    prev = lib.cpc_gemm_set_mode(1)
    try:
        cv = torch.empty(virt, cols, device=DEV)
        _lib.check(lib.cpc_gemm_nt(_lib.ptr(yd), stride * H, _lib.ptr(wd), K, _lib.ptr(cv), cols, _lib.ptr(bd), virt, cols, K,
                                   _lib.stream_ptr(c.device)))
    finally:
        lib.cpc_gemm_set_mode(prev)
    emax = {"planes": 0.0, "f32": 0.0, "torch": 0.0}
    esq = {"planes": 0.0, "f32": 0.0, "torch": 0.0}
    for n in range(n_win):
        a32 = torch.as_strided(y, (frames, K), (stride * H, 1), n * R * H)
        a = a32.double()
        ref = a @ w.double().t() + bias.double()
        mag = (a.abs() @ w.double().abs().t() + bias.double().abs()).clamp_min(1e-300)
        ct = a32.contiguous().to(DEV) @ wd.t() + bd
        for name, got in (("planes", c[n * frames:(n + 1) * frames]), ("f32", cv[n * (R // stride):n * (R // stride) + frames]),
                          ("torch", ct)):
            e = (got.cpu().double() - ref).abs() / mag
            emax[name] = max(emax[name], float(e.max()))
            esq[name] += float(e.pow(2).mean()) / n_win
    yard_rms, yard_max = max(esq["f32"], esq["torch"]) ** 0.5, max(emax["f32"], emax["torch"])
    assert esq["planes"] ** 0.5 <= max(1.35 * yard_rms, SEQ_F32_RMS), (esq, emax)
    assert emax["planes"] <= max(1.5 * yard_max, 12 * SEQ_F32_RMS), (esq, emax)
    assert emax["planes"] <= 16 * 2.0 ** -24


@pytest.mark.parametrize("stride,taps,n_rows,data", [(4, 8, 5 * 132, "relu"), (1, 1, 3000, "randn"), (2, 4, 64, "tiny")])
def test_plane_fed_gemm_tn_accuracy(stride, taps, n_rows, data):
    """cpc_gemm_tn_planes: the weight gradient of a strided Conv1d, dW[co][j * H + ci] = sum_m dU[m + 1][co] * Y[m * s + j][ci],
    from the stored planes of dU and Y -- vs fp64 and vs the f32-MFMA kernel (cpc_gemm_tn, mode 1), and bitwise
    repeatable (the row slabs are summed in a fixed order)."""
    lib = _lib.load()
    H = 256
    g = torch.Generator().manual_seed(stride * 100 + n_rows)
    K = taps * H
    rows = ((n_rows + 63) // 64 * 64 + 2) * stride + taps          # (the kernel reads whole 32-row slabs: finite rows behind R)
    rows = (rows + stride - 1) // stride * stride
    y = torch.randn(rows, H, generator=g)
    if data == "relu":
        y = y.clamp_min(0)
    rowsd = (n_rows + 2 + 63) // 32 * 32
    du = torch.randn(rowsd, H, generator=g) * 0.1
    du[n_rows + 1:] = 0
    if data == "tiny":
        y, du = y * 1e-7, du * 1e-9
    yd, dud = y.to(DEV), du.to(DEV)
    sl = stride.bit_length() - 1
    yp, ya, rts = _to_planes(lib, yd, sl)
    dup, da, _ = _to_planes(lib, dud)
    st = _lib.stream_ptr(yd.device)
    nb = lib.cpc_gemm_tn_planes_scratch_bytes(H, K, n_rows)
    sc = torch.empty(max(nb, 1), dtype=torch.uint8, device=DEV)
    outs = []
    for _ in range(2):
        dw = torch.empty(H, K, device=DEV)
        _lib.check(lib.cpc_gemm_tn_planes(_lib.ptr(dup), da, 0, rowsd, 1, H, _lib.ptr(yp), ya, sl, rts, 0, H, _lib.ptr(dw), K, H, K,
                                          n_rows, _lib.ptr(sc), nb, st))
        outs.append(dw.cpu())
    assert torch.equal(outs[0], outs[1])
    a = torch.as_strided(y, (n_rows, K), (stride * H, 1), 0).double()
    d = du[1:1 + n_rows].double()
    ref, mag = d.t() @ a, (d.abs().t() @ a.abs()).clamp_min(1e-300)
    prev = lib.cpc_gemm_set_mode(1)
    try:
        nb2 = lib.cpc_gemm_tn_scratch_bytes(H, K, n_rows)
        sc2 = torch.empty(max(nb2, 1), dtype=torch.uint8, device=DEV)
        dw2 = torch.empty(H, K, device=DEV)
        _lib.check(lib.cpc_gemm_tn(_lib.ptr(dud[1:]), H, _lib.ptr(yd), stride * H, _lib.ptr(dw2), K, H, K, n_rows, _lib.ptr(sc2), nb2, st))
    finally:
        lib.cpc_gemm_set_mode(prev)
    a32 = torch.as_strided(y, (n_rows, K), (stride * H, 1), 0).contiguous().to(DEV)
    dwt = dud[1:1 + n_rows].t() @ a32                               # torch's f32 matmul: the second yardstick (see the NT test)
    e_pl = (outs[0].double() - ref).abs() / mag
    e_32 = (dw2.cpu().double() - ref).abs() / mag
    e_t = (dwt.cpu().double() - ref).abs() / mag
    yard_rms = max(float(e_32.pow(2).mean().sqrt()), float(e_t.pow(2).mean().sqrt()))
    yard_max = max(float(e_32.max()), float(e_t.max()))
    assert float(e_pl.pow(2).mean().sqrt()) <= max(1.35 * yard_rms, SEQ_F32_RMS), (float(e_pl.pow(2).mean().sqrt()), yard_rms)
    assert float(e_pl.max()) <= max(1.5 * yard_max, 12 * SEQ_F32_RMS), (float(e_pl.max()), yard_max)
    assert float(e_pl.max()) <= 16 * 2.0 ** -24


def test_gemm_split_specials():
    """inf / nan operands poison exactly the outputs they feed; zeros and denormal-range values are harmless."""
    lib = _lib.load()
    a = torch.randn(256, 64)
    b = torch.randn(128, 64)
    a[3, 5] = float("inf")
    a[7, 9] = float("nan")
    a[11, :] = 0.0
    a[12, :] = 1e-41
    c = torch.empty(256, 128, device=DEV)
    ad, bd = a.to(DEV), b.to(DEV)
    _lib.check(lib.cpc_gemm_nt(_lib.ptr(ad), 64, _lib.ptr(bd), 64, _lib.ptr(c), 128, None, 256, 128, 64, _lib.stream_ptr(c.device)))
    c = c.cpu()
    assert not torch.isfinite(c[3]).any() and torch.isnan(c[7]).all()
    assert (c[11] == 0).all() and torch.isfinite(c[12]).all() and c[12].abs().max() < 1e-38
    keep = torch.ones(256, dtype=torch.bool)
    keep[[3, 7]] = False
    assert torch.isfinite(c[keep]).all()


# ----------------------------------------------------------------------------- ChannelNorm (standalone, channel-first)
def test_channelnorm_module_vs_reference_golden(golden):
    g = golden("g3_channelnorm.npz")
    cn = cpc2_amd.ChannelNorm(16).to(DEV)
    cn.weight.data.copy_(t(g["w"]))
    cn.bias.data.copy_(t(g["b"]))
    x = t(g["x"]).to(DEV).requires_grad_(True)
    y = cn(x)
    (y * t(g["g"]).to(DEV)).sum().backward()
    assert_close(y, t(g["y"]), 1e-5, "y")
    assert_close(x.grad, t(g["dx"]), 2e-5, "dx")
    assert_close(cn.weight.grad, t(g["dw"]), 2e-5, "dw")
    assert_close(cn.bias.grad, t(g["db"]), 2e-5, "db")


# ----------------------------------------------------------------------------- encoder
def test_encoder_vs_reference_golden(golden):
    g = golden("g2_encoder_h32.npz")
    hidden = int(g["hidden"])
    enc = load_encoder(hidden, synth.encoder_params(hidden, int(g["param_seed"])))
    x = synth.audio_windows(2, 20480, int(g["x_seed"])).to(DEV)
    out = enc(x)
    assert out.shape == (2, hidden, 128)
    assert_close(out, t(g["out"]), 2e-5, "encoder output")
    (out * synth.features((2, hidden, 128), int(g["gout_seed"])).to(DEV)).sum().backward()
    for name, p in enc.named_parameters():
        assert_close(p.grad, t(g["grad." + name]), 1e-4, f"grad {name}")


# (256, 44, 20480): conv1's product has more than 160 tiles and does not split K -> ChannelNorm + ReLU + split in its epilogue
# (256, 43, 19800): the same with frame counts that are no multiple of the tile (990 per window: tiles straddle windows, the last is partial)
# lengths 159 .. 399: one and two frames, what the non-strict rest of a file feeds on its own (feature_loader.buildFeature); 159 is
# the shortest input the reference's Conv1d stack takes.  Forward only: the backward refuses them by name
# (32, 512, 2560): the f32 path's backward data of conv1 as TWO products -- the main one over the 128 frame rows of every window, one
# row per window for the boundary row (512 tiles against 513: rounds_seg < rounds_full in encoder_backward) -- and (32, 504, 2560),
# which stays on the single product; 1.2e7 pre-activations, so held like the many-window plane cases below
_SHORT_ENCODER_INPUTS = [(hidden, n, length) for hidden in (32, 256, 512)
                         for n, length in ((1, 159), (3, 160), (1, 319), (2, 320), (1, 399))] + [(64, 1, 159), (128, 2, 319)]


@pytest.mark.parametrize("hidden,n,length", [(256, 3, 20480), (64, 2, 3300), (512, 2, 4800), (128, 1, 20480), (256, 44, 20480),
                                             (256, 43, 19800), (32, 512, 2560), (32, 504, 2560)] + _SHORT_ENCODER_INPUTS)
def test_encoder_vs_oracle_fp64(hidden, n, length):
    from test_encoder_abi_gpu import two_product_layers            # enc_layout and the branch conditions, restated
    assert two_product_layers(hidden, n, length) == ([1] if (hidden, n, length) == (32, 512, 2560) else [])
    params = synth.encoder_params(hidden, seed=5)
    enc = load_encoder(hidden, params)
    x = synth.audio_windows(n, length, seed=6)
    p64 = {k: v.double().requires_grad_(True) for k, v in params.items()}
    ref = O.encoder_forward(x.double(), p64, "gEncoder.")
    gout = synth.features(tuple(ref.shape), seed=7)
    (ref * gout.double()).sum().backward()
    out = enc(x.to(DEV))
    assert tuple(out.shape) == tuple(ref.shape)
    assert_close(out, ref, 2e-5, "encoder output")
    if length < 400:
        assert tuple(out.shape) == (n, hidden, 1 if length < 319 else 2)
        with pytest.raises(ValueError, match="encoder_backward: inputs shorter than 400 samples are forward-only"):
            (out * gout.to(DEV)).sum().backward()
        return
    (out * gout.to(DEV)).sum().backward()
    # Many windows: the gradients below a layer are conditioned by that layer's ReLU decisions.  Of ~6e7 pre-activations a
    # handful lie within fp32 rounding of zero and fall the other way in ANY fp32 evaluation than in fp64; each such decision
    # changes the gradients below it by whole terms of sums that (under a random upstream gradient) cancel to ~1 / sqrt(terms)
    # of their terms: one decision in layer 0 moves conv0.weight.grad by ~1e-3 of its largest element.  That says nothing about
    # the arithmetic, so it is taken out of the comparison instead of being tolerated: the kernels' own ReLU decisions are read
    # back (the layer outputs the forward pass keeps: cpc_encoder_saved_layout) and the fp64 oracle is differentiated WITH THOSE
    # decisions -- then every gradient must agree to 5e-5 (measured <= 1.0e-5 at 43 / 44 windows with 1 / 3 decisions that differ,
    # each of which alone accounts for the 7e-4 .. 7e-3 of the unconditioned comparison).  Separately: the decisions differ
    # from fp64's own in at most 1e-6 of the elements, and only where the fp64 pre-activation is within 1e-5 of zero.  The
    # unconditioned comparison stays as a coarse end-to-end gate (2e-2).
    if n <= 16:
        for name, p in enc.named_parameters():
            assert_close(p.grad, p64["gEncoder." + name].grad, 2e-4, f"grad {name}")
        return
    for name, p in enc.named_parameters():
        assert rel_err(p.grad, p64["gEncoder." + name].grad) <= 2e-2, f"grad {name} (coarse gate)"
    masks = _kernel_relu_decisions(hidden, params, x)
    pm = {k: v.double().requires_grad_(True) for k, v in params.items()}
    pre = []
    refm = O.encoder_forward(x.double(), pm, "gEncoder.", masks=masks, pre_out=pre)
    (refm * gout.double()).sum().backward()
    flips = 0
    for i, (m, y) in enumerate(zip(masks, pre)):
        diff = m.bool() != (y > 0)
        flips += int(diff.sum())
        assert float(diff.float().mean()) <= 1e-6, f"layer {i}: {int(diff.sum())} ReLU decisions differ from the fp64 oracle's"
        if diff.any():
            worst = float(y[diff].abs().max() / y.abs().max())
            assert worst <= 1e-5, f"layer {i}: a pre-activation of relative size {worst:.2e} was decided the other way"
    print(f"ReLU decisions that differ from fp64's: {flips}")
    for name, p in enc.named_parameters():
        print(f"{name}: unconditioned {rel_err(p.grad, p64['gEncoder.' + name].grad):.2e}, same decisions {rel_err(p.grad, pm['gEncoder.' + name].grad):.2e}")
    for name, p in enc.named_parameters():
        assert_close(p.grad, pm["gEncoder." + name].grad, 5e-5, f"grad {name} (the kernels' ReLU decisions)")


@pytest.mark.parametrize("hidden,n,n_first", [(256, 5, 2), (64, 3, 1), (512, 4, 3)])
def test_encoder_over_two_input_batches_equals_the_concatenated_call(hidden, n, n_first):
    """cpc_encoder_forward / cpc_encoder_backward with x_rest: windows 0 .. n_first - 1 from one buffer, the rest from another (train.py:99's
    cat([past, future]) as two pointers; only conv0's kernels read the waveform): output and every gradient are those of the
    concatenated call, bit for bit."""
    params = synth.encoder_params(hidden, seed=5)
    x = synth.audio_windows(n, 20480, seed=6).to(DEV)
    gout = synth.features((n, 128, hidden), seed=7).to(DEV)
    res = []
    for pair in (False, True):
        enc = load_encoder(hidden, params)
        out = enc.forward_channel_last(x[:n_first].clone(), x[n_first:].clone()) if pair else enc.forward_channel_last(x)
        (out * gout).sum().backward()
        res.append((out.detach().clone(), {k: p.grad.clone() for k, p in enc.named_parameters()}))
    assert torch.equal(res[0][0], res[1][0])
    for k in res[0][1]:
        assert torch.equal(res[0][1][k], res[1][1][k]), k
    with pytest.raises(ValueError):
        enc.forward_channel_last(x[:1], x[1:, :, :100].contiguous())


def _kernel_relu_decisions(hidden, params, x, windows=None):
    """The 0/1 masks [N, H, L_i] of the five ReLUs as the HIP forward pass decided them, read from what it keeps: the outputs
    of layers 0..3 are the next layers' input in `saved` (cpc_encoder_saved_layout: bf16 planes at hidden 256 / 512, f32 rows
    below), layer 4's is z.  windows: only
    these windows' masks (the forward pass still runs on all of x: the launch geometry is the batch's)."""
    lib = _lib.load()
    n, _one, length = x.shape
    sel = torch.arange(n, device=DEV) if windows is None else torch.as_tensor(list(windows), device=DEV)
    plist = [v.to(DEV).contiguous() for v in params.values()]
    xd = x.to(DEV)
    frames = lib.cpc_encoder_frames(length)
    z = torch.empty(n, frames, hidden, device=DEV)
    saved = torch.zeros(lib.cpc_encoder_saved_bytes(n, length, hidden), dtype=torch.uint8, device=DEV)
    scratch = torch.empty(lib.cpc_encoder_scratch_bytes(n, length, hidden), dtype=torch.uint8, device=DEV)
    _lib.check(lib.cpc_encoder_forward(_lib.ptr(xd), None, n, _lib.ptr_array(plist), _lib.ptr(z), _lib.ptr(saved), _lib.ptr(scratch), n, length,
                                       hidden, 1e-5, _lib.stream_ptr(xd.device)), "encoder_forward")
    masks = []
    for layer in range(4):
        lay = (ctypes.c_long * 10)()
        _lib.check(lib.cpc_encoder_saved_layout(n, length, hidden, layer, lay), "saved_layout")
        _xo, _ro, _rv, lv, po, plane, rts, sshift, rows_next, halo = list(lay)
        if hidden % 256 != 0:                      # f32 rows: [5] is their byte offset, row n * rows_next + halo + t
            assert po == -1 and plane >= 0 and rows_next >= halo + lv and rts == 0 and sshift == 0
            y = saved[plane:plane + 4 * n * rows_next * hidden].view(torch.float32).view(n, rows_next, hidden)[sel, halo:halo + lv]
            masks.append((y > 0).permute(0, 2, 1).contiguous().cpu())
            continue
        assert po >= 0
        planes = saved[po:po + 2 * 3 * plane].view(torch.bfloat16).view(3, plane)
        ch = torch.arange(hidden, device=DEV).view(1, 1, hidden)
        R = (sel.view(-1, 1, 1) * rows_next + halo + torch.arange(lv, device=DEV).view(1, lv, 1))
        idx = ((((ch // 16) << sshift) + (R & ((1 << sshift) - 1))) * rts + (R >> sshift)) * 16 + ch % 16      # [n, lv, hidden]
        y = (planes[0][idx].float() + planes[1][idx].float()) + planes[2][idx].float()
        masks.append((y > 0).permute(0, 2, 1).contiguous().cpu())
        del idx, y, R
    masks.append((z[sel] > 0).permute(0, 2, 1).contiguous().cpu())
    return masks


_ENC_FORMS_SCRIPT = """
import sys, torch
sys.path.insert(0, {root!r})
import cpc2_amd
from oracle import synth
hidden, n = 256, {n}
enc = cpc2_amd.CPCEncoder(hidden)
enc.load_state_dict({{k[len("gEncoder."):]: v for k, v in synth.encoder_params(hidden, seed=5).items()}})
enc = enc.to("cuda:0")
x = synth.audio_windows(n, 20480, seed=6).to("cuda:0")
out = enc(x)
(out * synth.features(tuple(out.shape), seed=7).to("cuda:0")).sum().backward()
torch.save({{"out": out.detach().cpu(), **{{k: p.grad.cpu() for k, p in enc.named_parameters()}}}}, {dst!r})
"""


def test_encoder_with_and_without_the_fused_norm_epilogue(tmp_path):
    """96 windows at hidden 256: conv1 AND conv2 run without a K split, so both take ChannelNorm + ReLU + split in the product's
    epilogue (gemm_nt_planes with a PlanesNormOut).  CPC_NO_NORM_FUSION=1 (read once per process) gives the three-kernel form the
    oracle tests cover at small window counts; the two agree to fp32 rounding in the output and in every gradient."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for form, env in (("fused", {}), ("plain", {"CPC_NO_NORM_FUSION": "1"})):
        dst = str(tmp_path / f"{form}.pt")
        e = dict(os.environ, PYTHONPATH=root, **env)
        if form == "fused":
            e.pop("CPC_NO_NORM_FUSION", None)
        r = subprocess.run([sys.executable, "-c", _ENC_FORMS_SCRIPT.format(root=root, n=96, dst=dst)], env=e, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[form] = torch.load(dst)
    # (gradients: see the conditioning note in test_encoder_vs_oracle_fp64 -- two fp32 evaluation orders differ by ~1e-3 there)
    for key in res["plain"]:
        tol = 1e-2 if key != "out" else 2e-5
        e = rel_err(res["fused"][key], res["plain"][key].double())
        print(f"{key}: {e:.2e}")
        assert e <= tol, f"{key} (fused epilogue vs norm kernel): rel err {e:.3e} > {tol:.1e}"
    assert not torch.equal(res["fused"]["out"], res["plain"]["out"]), "the switch selected the same kernels twice"


@pytest.mark.parametrize("hidden,n", [(256, 128), (512, 16)])
def test_pair_form_of_the_plane_fed_kernel_is_bit_identical_to_the_one_tap_form(tmp_path, hidden, n):
    """The pair form (A tile of a tap pair staged once, second tap's fragments read one row down; conv1-3 forward and backward
    data at the training window length, with and without a K split, with and without the fused norm epilogue) multiplies the
    same fragments in the same order as the one-tap-per-stage form (CPC_PLANES_NO_PAIR=1, its own process): the encoder's output
    and every gradient are equal bit for bit."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    script = _ENC_FORMS_SCRIPT.replace("hidden, n = 256, {n}", "hidden, n = {hidden}, {n}")
    for form, env in (("pair", {}), ("one_tap", {"CPC_PLANES_NO_PAIR": "1"})):
        dst = str(tmp_path / f"{form}.pt")
        e = dict(os.environ, PYTHONPATH=root, **env)
        if form == "pair":
            e.pop("CPC_PLANES_NO_PAIR", None)
        r = subprocess.run([sys.executable, "-c", script.format(root=root, hidden=hidden, n=n, dst=dst)], env=e, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[form] = torch.load(dst)
    for key in res["one_tap"]:
        assert torch.equal(res["pair"][key], res["one_tap"][key]), f"{key}: the two forms differ (max {float((res['pair'][key] - res['one_tap'][key]).abs().max()):.3e})"
    assert float(res["pair"]["out"].abs().max()) > 0


_ENC_SAVED_SCRIPT = """
import ctypes, sys, torch
sys.path.insert(0, {root!r})
from cpc2_amd import _lib
from oracle import synth
lib = _lib.load()
hidden, n, length = 256, {n}, {length}
dev = torch.device("cuda:0")
params = [v.to(dev).contiguous() for v in synth.encoder_params(hidden, seed=5).values()]
x = synth.audio_windows(n, length, seed=6).to(dev)
frames = lib.cpc_encoder_frames(length)
z = torch.empty(n, frames, hidden, device=dev)
saved = torch.zeros(lib.cpc_encoder_saved_bytes(n, length, hidden), dtype=torch.uint8, device=dev)
scratch = torch.empty(lib.cpc_encoder_scratch_bytes(n, length, hidden), dtype=torch.uint8, device=dev)
_lib.check(lib.cpc_encoder_forward(_lib.ptr(x), None, n, _lib.ptr_array(params), _lib.ptr(z), _lib.ptr(saved), _lib.ptr(scratch), n, length,
                                   hidden, 1e-5, _lib.stream_ptr(dev)), "encoder_forward")
torch.cuda.synchronize()
out = {{"z": z.cpu()}}
for layer in (1, 2, 3):
    lay = (ctypes.c_long * 10)()
    _lib.check(lib.cpc_encoder_saved_layout(n, length, hidden, layer, lay), "saved_layout")
    xo, ro, rv, lv, po, plane, rts, sshift, _rn, _halo = list(lay)
    xh = saved[xo:xo + 4 * n * rv * hidden].view(torch.float32).view(n, rv, hidden)[:, :lv]
    rstd = saved[ro:ro + 4 * n * rv].view(torch.float32).view(n, rv)[:, :lv]
    out[f"xhat{{layer}}"], out[f"rstd{{layer}}"] = xh.cpu(), rstd.cpu()
    planes = saved[po:po + 2 * 3 * plane].view(torch.bfloat16).view(3, plane)
    out[f"planes{{layer}}"] = planes.cpu().view(torch.int16)          # the three terms as stored (halo and slack rows included)
torch.save(out, {dst!r})
"""


@pytest.mark.parametrize("n,length", [(44, 20480), (96, 20480), (43, 19800)])
def test_fused_norm_epilogue_saves_the_same_state_as_the_norm_kernel(tmp_path, n, length):
    """What the fused epilogue of conv1 / conv2 (gemm_planes_kernel<0, false, 6, true>) leaves for the backward pass and for the
    next layer, read straight out of `saved` (cpc_encoder_saved_layout) and compared with the three-kernel form
    (CPC_NO_NORM_FUSION=1, its own process: the switch is read once) -- model.py:52-60's statistics, not their effect on a
    gradient: xhat and rstd of every valid row to 1e-6 (1e-5 of the largest element for single elements of xhat), and the next
    layer's input planes, halo and slack rows included: their sum p0 + p1 + p2 equal to 1e-6, zero rows zero in both.
    Layer 3 is the norm kernel in both forms (its product splits K); its input differs by the rounding above."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for form, env in (("fused", {}), ("plain", {"CPC_NO_NORM_FUSION": "1"})):
        dst = str(tmp_path / f"{form}.pt")
        e = dict(os.environ, PYTHONPATH=root, **env)
        if form == "fused":
            e.pop("CPC_NO_NORM_FUSION", None)
        r = subprocess.run([sys.executable, "-c", _ENC_SAVED_SCRIPT.format(root=root, n=n, length=length, dst=dst)], env=e,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[form] = torch.load(dst)
    f, p = res["fused"], res["plain"]
    assert_close(f["z"], p["z"], 2e-6, "encoder output")
    for layer in (1, 2):
        for key in (f"xhat{layer}", f"rstd{layer}"):
            a, b = f[key].double(), p[key].double()
            assert torch.isfinite(a).all()
            e_max = float((a - b).abs().max() / b.abs().max())
            e_rms = float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())
            print(f"{key}: max {e_max:.2e} rms {e_rms:.2e}")
            assert e_rms <= 1e-6 and e_max <= (1e-6 if key.startswith("rstd") else 1e-5), f"{key}: rms {e_rms:.2e}, max {e_max:.2e}"
        # per-row rstd: relative, element by element (a row's statistic is one number: nothing to average over)
        rel = ((f[f"rstd{layer}"].double() - p[f"rstd{layer}"].double()).abs() / p[f"rstd{layer}"].double().abs()).max()
        assert float(rel) <= 2e-6, f"rstd{layer}: worst row off by {float(rel):.2e} relative"
        # (p0 + p1 + p2 is an f32 by construction: the f32 sum is exact.  A ReLU decision that falls the other way for a
        #  pre-activation within rounding of zero shows as a difference of that size; a halo or slack row that one form left
        #  non-zero would show as O(1))
        pa, pb = f[f"planes{layer}"].view(torch.bfloat16).float(), p[f"planes{layer}"].view(torch.bfloat16).float()
        ya, yb = (pa[0] + pa[1]) + pa[2], (pb[0] + pb[1]) + pb[2]
        assert float(((ya == 0) != (yb == 0)).float().mean()) <= 1e-5, f"layer {layer}: zero pattern of the next layer's input differs"
        e_y = float((ya - yb).abs().max() / yb.abs().max())
        print(f"planes{layer}: max {e_y:.2e}")
        assert e_y <= 1e-6, f"planes{layer}: p0 + p1 + p2 differs by {e_y:.2e}"
    assert not torch.equal(f["xhat1"], p["xhat1"]), "the switch selected the same kernels twice"
    assert_close(f["xhat3"], p["xhat3"], 1e-5, "xhat3")


# ----------------------------------------------------------------------------- GRU
def load_ar(hin, hid, layers, params, reverse=False, keep=False):
    ar = cpc2_amd.CPCAR(hin, hid, keep, layers, mode="GRU", reverse=reverse)
    ar.load_state_dict({k[len("gAR."):]: v for k, v in params.items()})
    return ar.to(DEV)


@pytest.mark.parametrize("tag", ["l1", "l2"])
def test_gru_vs_reference_golden(golden, tag):
    g = golden("g4_gru.npz")
    hin, hid, layers, n, t_len = (int(v) for v in g[f"{tag}_cfg"])
    ar = load_ar(hin, hid, layers, synth.gru_params(hin, hid, layers, 41))
    x = synth.features((n, t_len, hin), 42, relu=True).to(DEV).requires_grad_(True)
    out = ar(x)
    assert_close(out, t(g[f"{tag}_out"]), 1e-5, "gru out")
    (out * synth.features((n, t_len, hid), 43).to(DEV)).sum().backward()
    assert_close(x.grad, t(g[f"{tag}_dx"]), 1e-4, "gru dx")
    for name, p in ar.named_parameters():
        assert_close(p.grad, t(g[f"{tag}_grad." + name]), 1e-4, f"gru grad {name}")


def test_gru_reverse_and_keep_hidden(golden):
    g = golden("g4_gru.npz")
    params = synth.gru_params(32, 32, 1, 41)
    x = synth.features((3, 20, 32), 42, relu=True).to(DEV)
    assert_close(load_ar(32, 32, 1, params, reverse=True)(x), t(g["rev_out"]), 1e-5, "reverse")
    # keepHidden: two half-sequences with carried state == one full sequence (model.py:197-201)
    full = load_ar(32, 32, 1, params)(x)
    ar = load_ar(32, 32, 1, params, keep=True)
    halves = torch.cat([ar(x[:, :10].contiguous()), ar(x[:, 10:].contiguous())], dim=1)
    assert_close(halves, full, 1e-6, "keepHidden")


# window counts chosen to reach every windows-per-group variant of the cooperative kernels (H = 256: 64 groups of 4 CUs,
# H = 512: 16 groups of 16 CUs) and a ragged last group
@pytest.mark.parametrize("hid,layers,n,t_len", [(256, 1, 5, 128), (512, 2, 3, 40), (512, 1, 100, 12), (512, 1, 40, 10),
                                                (512, 1, 20, 9), (256, 1, 300, 6), (256, 2, 130, 7), (512, 2, 128, 21),
                                                (512, 1, 128, 1), (256, 1, 128, 2), (512, 1, 65, 3)])       # (sequence ends: no hand-off, one)
def test_gru_vs_oracle_fp64(hid, layers, n, t_len):
    params = synth.gru_params(hid, hid, layers, 9)
    ar = load_ar(hid, hid, layers, params)
    x = synth.features((n, t_len, hid), 10, relu=True)
    p64 = {k: v.double().requires_grad_(True) for k, v in params.items()}
    x64 = x.double().requires_grad_(True)
    ref, _ = O.gru_forward(x64, p64, layers, "gAR.baseNet.")
    gout = synth.features((n, t_len, hid), 11)
    (ref * gout.double()).sum().backward()
    xd = x.to(DEV).requires_grad_(True)
    out = ar(xd)
    assert_close(out, ref, 1e-5, "gru out")
    (out * gout.to(DEV)).sum().backward()
    assert_close(xd.grad, x64.grad, 1e-4, "gru dx")
    for name, p in ar.named_parameters():
        assert_close(p.grad, p64["gAR." + name].grad, 1e-4, f"gru grad {name}")


# What feature extraction feeds the context network for a rest of 159 .. 399 samples: one window (or a few) of one or two frames
@pytest.mark.parametrize("t_len", [1, 2])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("mode,hid,layers", [("GRU", 32, 1), ("GRU", 256, 1), ("GRU", 512, 2), ("LSTM", 32, 1), ("LSTM", 256, 2),
                                             ("LSTM", 512, 1), ("RNN", 32, 2), ("RNN", 256, 1), ("RNN", 512, 1),
                                             ("transformer", 64, 1), ("transformer", 256, 1), ("transformer", 512, 1)])
def test_context_networks_on_one_and_two_frames_vs_oracle_fp64(mode, hid, layers, n, t_len):
    x = synth.features((n, t_len, hid), 10, relu=True)
    if mode == "transformer":
        params = synth.transformer_params(hid, hid, 128, 81)
        net = load_transformer(hid, hid, 128, params).eval()
        ref = O.transformer_layer_forward(x.double(), to64(params), "gAR.0.", size_seq=128)
        tol = 2e-5
    else:
        make, fwd = {"GRU": (synth.gru_params, O.gru_forward), **_RECURRENT}[mode]
        params = make(hid, hid, layers, 9)
        net = cpc2_amd.CPCAR(hid, hid, False, layers, mode=mode)
        net.load_state_dict({k[len("gAR."):]: v for k, v in params.items()})
        net = net.to(DEV).eval()
        ref = fwd(x.double(), to64(params), layers, "gAR.baseNet.")[0]
        tol = 1e-5
    with torch.no_grad():
        out = net(x.to(DEV))
    assert tuple(out.shape) == (n, t_len, hid)
    assert_close(out, ref, tol, f"{mode} on {t_len} frame(s)")


_GRU_FORMS_SCRIPT = """
import sys, torch
sys.path.insert(0, {root!r})
import cpc2_amd
from oracle import synth
hid, n, t_len = {hid}, {n}, {t_len}
params = synth.gru_params(hid, hid, 1, 9)
ar = cpc2_amd.CPCAR(hid, hid, False, 1)
ar.load_state_dict({{k[len("gAR."):]: v for k, v in params.items()}})
ar = ar.to("cuda:0")
x = synth.features((n, t_len, hid), 10, relu=True).to("cuda:0").requires_grad_(True)
out = ar(x)
(out * synth.features((n, t_len, hid), 11).to("cuda:0")).sum().backward()
torch.save({{"out": out.detach().cpu(), "dx": x.grad.cpu(), **{{k: p.grad.cpu() for k, p in ar.named_parameters()}}}}, {dst!r})
"""


@pytest.mark.parametrize("hid,n,t_len", [(256, 128, 9), (512, 24, 7)])
def test_gru_matrix_pipe_and_valu_forms_agree(tmp_path, hid, n, t_len):
    """Both forms of the cooperative GRU step (FMAs on the member's register-resident weights; the exact bf16 split on the
    matrix pipe) at window counts where only ONE of them is the default: CPC_GRU_MFMA_ALL / CPC_GRU_NO_MFMA select them (read
    once per process, hence the child processes), and they agree to fp32 rounding."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for form, env in (("mfma", {"CPC_GRU_MFMA_ALL": "1"}), ("valu", {"CPC_GRU_NO_MFMA": "1"})):
        dst = str(tmp_path / f"{form}.pt")
        e = dict(os.environ, PYTHONPATH=root, **env)
        e.pop("CPC_GRU_NO_MFMA" if form == "mfma" else "CPC_GRU_MFMA_ALL", None)
        r = subprocess.run([sys.executable, "-c", _GRU_FORMS_SCRIPT.format(root=root, hid=hid, n=n, t_len=t_len, dst=dst)], env=e,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        res[form] = torch.load(dst)
    for key in res["valu"]:
        assert_close(res["mfma"][key], res["valu"][key].double(), 2e-5, f"{key} (matrix pipe vs FMA form)")
    assert not torch.equal(res["mfma"]["out"], res["valu"]["out"]), "the switch selected the same kernels twice"


# ----------------------------------------------------------------------------- LSTM / RNN (model.py:171-176)
_RECURRENT = {"LSTM": (synth.lstm_params, O.lstm_forward), "RNN": (synth.rnn_params, O.rnn_forward)}


def load_recurrent(mode, hin, hid, layers, params, reverse=False, keep=False):
    ar = cpc2_amd.CPCAR(hin, hid, keep, layers, mode=mode, reverse=reverse)
    ar.load_state_dict({k[len("gAR."):]: v for k, v in params.items()})
    return ar.to(DEV)


@pytest.mark.parametrize("mode", ["LSTM", "RNN"])
@pytest.mark.parametrize("tag", ["l1", "l2"])
def test_lstm_rnn_vs_reference_golden(golden, mode, tag):
    g = golden("g12_lstm_rnn.npz")
    hin, hid, layers, n, t_len = (int(v) for v in g[f"{mode}_{tag}_cfg"])
    ar = load_recurrent(mode, hin, hid, layers, _RECURRENT[mode][0](hin, hid, layers, 51))
    x = synth.features((n, t_len, hin), 52, relu=True).to(DEV).requires_grad_(True)
    out = ar(x)
    assert_close(out, t(g[f"{mode}_{tag}_out"]), 1e-5, f"{mode} out")
    (out * synth.features((n, t_len, hid), 53).to(DEV)).sum().backward()
    assert_close(x.grad, t(g[f"{mode}_{tag}_dx"]), 1e-4, f"{mode} dx")
    for name, p in ar.named_parameters():
        assert_close(p.grad, t(g[f"{mode}_{tag}_grad." + name]), 1e-4, f"{mode} grad {name}")


@pytest.mark.parametrize("mode", ["LSTM", "RNN"])
def test_lstm_rnn_keep_hidden_vs_reference_golden(golden, mode):
    g = golden("g12_lstm_rnn.npz")
    ar = load_recurrent(mode, 32, 32, 2, _RECURRENT[mode][0](32, 32, 2, 51), keep=True)
    ar(synth.features((2, 9, 32), 54, relu=True).to(DEV))
    out2 = ar(synth.features((2, 7, 32), 55, relu=True).to(DEV))
    assert_close(out2, t(g[f"{mode}_keep_out2"]), 1e-5, "second call")
    if mode == "LSTM":
        assert isinstance(ar.hidden, tuple) and len(ar.hidden) == 2
        assert_close(ar.hidden[0], t(g["LSTM_keep_h"]), 1e-5, "h")
        assert_close(ar.hidden[1], t(g["LSTM_keep_c"]), 1e-5, "c")
    else:
        assert_close(ar.hidden, t(g["RNN_keep_h"]), 1e-5, "h")


@pytest.mark.parametrize("mode,hin,hid,layers,n,t_len", [("LSTM", 256, 256, 1, 5, 128), ("LSTM", 512, 512, 2, 3, 40),
                                                         ("LSTM", 256, 256, 2, 70, 12), ("LSTM", 64, 100, 1, 4, 17),
                                                         ("LSTM", 512, 512, 1, 100, 12), ("LSTM", 512, 512, 1, 40, 10),
                                                         ("LSTM", 256, 256, 1, 300, 6), ("LSTM", 128, 256, 2, 130, 7),
                                                         ("LSTM", 256, 256, 1, 2000, 3),
                                                         ("RNN", 256, 256, 1, 5, 128), ("RNN", 512, 512, 2, 3, 40),
                                                         ("RNN", 48, 36, 2, 9, 11)])
def test_lstm_rnn_vs_oracle_fp64(mode, hin, hid, layers, n, t_len):
    make, fwd = _RECURRENT[mode]
    params = make(hin, hid, layers, 9)
    ar = load_recurrent(mode, hin, hid, layers, params)
    x = synth.features((n, t_len, hin), 10, relu=True)
    p64 = {k: v.double().requires_grad_(True) for k, v in params.items()}
    x64 = x.double().requires_grad_(True)
    ref = fwd(x64, p64, layers, "gAR.baseNet.")[0]
    gout = synth.features((n, t_len, hid), 11)
    (ref * gout.double()).sum().backward()
    xd = x.to(DEV).requires_grad_(True)
    out = ar(xd)
    assert_close(out, ref, 1e-5, f"{mode} out")
    (out * gout.to(DEV)).sum().backward()
    assert_close(xd.grad, x64.grad, 1e-4, f"{mode} dx")
    for name, p in ar.named_parameters():
        assert_close(p.grad, p64["gAR." + name].grad, 1e-4, f"{mode} grad {name}")


@pytest.mark.parametrize("hid,n", [(256, 6), (512, 21), (96, 3)])
def test_lstm_keep_hidden_halves_equal_full_sequence(hid, n):
    """keepHidden (model.py:197-201): two half-sequences with the carried (h, c) == one full sequence, on the
    cooperative (256, 512) and the streaming (96) kernels."""
    params = synth.lstm_params(hid, hid, 2, 5)
    x = synth.features((n, 24, hid), 6, relu=True).to(DEV)
    full = load_recurrent("LSTM", hid, hid, 2, params)(x)
    ar = load_recurrent("LSTM", hid, hid, 2, params, keep=True)
    halves = torch.cat([ar(x[:, :10].contiguous()), ar(x[:, 10:].contiguous())], dim=1)
    assert_close(halves, full, 1e-6, "keepHidden")


def test_lstm_reverse_matches_flipped_forward():
    params = synth.lstm_params(32, 32, 1, 3)
    x = synth.features((3, 20, 32), 4, relu=True).to(DEV)
    fwd = load_recurrent("LSTM", 32, 32, 1, params)(torch.flip(x, [1]))
    rev = load_recurrent("LSTM", 32, 32, 1, params, reverse=True)(x)
    assert torch.equal(rev, torch.flip(fwd, [1]))


# ----------------------------------------------------------------------------- criterion
def make_criterion(k, har, henc, nn, pseed, scale=4.0, **kw):
    crit = cpc2_amd.CPCUnsupersivedCriterion(k, har, henc, nn, rnnMode="linear", sizeInputSeq=999, **kw)
    crit.load_state_dict(synth.predictor_params(k, har, henc, seed=pseed, scale=scale))
    return crit.to(DEV)


@pytest.mark.parametrize("tag", ["plain", "skip", "reverse", "quality", "rect"])
def test_criterion_small_vs_reference_golden(golden, tag):
    g = golden("g5_criterion_small.npz")
    har = 24 if tag == "rect" else 32
    kw = {}
    if tag == "skip":
        kw["n_skipped"] = 1
    if tag == "reverse":
        kw["mode"] = "reverse"
    if tag == "quality":
        kw.update(growth_rate=2.0, inflection_point_x=0.1)
    crit = make_criterion(4, har, 32, 16, 50, **kw)
    c = synth.features((4, 32, har), 51).to(DEV).requires_grad_(True)
    z = synth.features((4, 32, 32), 52, relu=True).to(DEV).requires_grad_(True)
    quality = t(g["quality_signal"]).to(DEV) if tag == "quality" else None
    torch.manual_seed(99)                      # the reference drew its negatives from this CPU stream
    losses, acc = crit(c, z, None, quality)
    assert losses.shape == tuple(g[f"{tag}_losses"].shape)
    assert_close(losses, t(g[f"{tag}_losses"]), 2e-6, "losses")
    assert torch.allclose(acc.cpu(), t(g[f"{tag}_acc"]), atol=1.5 / (4 * 28))
    losses.sum().backward()
    assert_close(c.grad, t(g[f"{tag}_dc"]), 5e-5, "dc")
    assert_close(z.grad, t(g[f"{tag}_dz"]), 5e-5, "dz")
    for i in range(4):
        w = crit.wPrediction.predictors[i].weight
        ref = t(g[f"{tag}_dW{i}"])
        if float(ref.abs().max()) == 0.0:
            assert w.grad is None or float(w.grad.abs().max()) == 0.0
        else:
            assert_close(w.grad, ref, 5e-5, f"dW{i}")


def test_criterion_full_shape_vs_reference_golden(golden):
    """Config-C2 shapes (T=128, H=256, K=12, 128 negatives) at b=8; loss within 1e-3 relative (north_star)."""
    g = golden("g5_criterion_full.npz")
    crit = make_criterion(12, 256, 256, 128, 60)
    c = synth.features((8, 128, 256), 61).to(DEV).requires_grad_(True)
    z = synth.features((8, 128, 256), 62, relu=True).to(DEV).requires_grad_(True)
    torch.manual_seed(1234)
    losses, acc = crit(c, z, None)
    assert_close(losses, t(g["losses"]), 1e-5, "losses")          # far inside the 1e-3 requirement
    assert torch.allclose(acc.cpu(), t(g["acc"]), atol=3e-3)
    losses.sum().backward()
    assert_close(c.grad[:, :3, :8], t(g["dc_head"]), 1e-4, "dc head")
    assert_close(z.grad[:, :3, :8], t(g["dz_head"]), 1e-4, "dz head")
    assert_close(z.grad[:, -3:, :8], t(g["dz_tail"]), 1e-4, "dz tail")
    for name, ten in (("dc", c.grad), ("dz", z.grad)):
        got, ref = float(ten.double().abs().sum()), float(g[f"{name}_abs"])
        assert abs(got - ref) <= 1e-4 * ref, name
    for i in range(12):
        w = crit.wPrediction.predictors[i].weight.grad
        assert abs(float(w.double().abs().sum()) - float(g[f"dW{i}_abs"])) <= 1e-4 * float(g[f"dW{i}_abs"])
        assert_close(w[:4, :8], t(g[f"dW{i}_head"]), 2e-4, f"dW{i} head")
    # EVERY element of every gradient: the fp64 oracle on the same inputs and negatives (tests/test_oracle_golden.py pins
    # the oracle at this very case to the reference's heads, tails and sums)
    p64 = {n: v.double().requires_grad_(True) for n, v in synth.predictor_params(12, 256, 256, seed=60, scale=4.0).items()}
    c64 = synth.features((8, 128, 256), 61).double().requires_grad_(True)
    z64 = synth.features((8, 128, 256), 62, relu=True).double().requires_grad_(True)
    _, _, ext = negative_indices(MT19937(1234), 8, 128, 116, 128)
    ref_losses, _ = O.criterion_forward(c64, z64, O.predictor_list(p64, 12), ext, 128)
    ref_losses.sum().backward()
    assert_close(losses, ref_losses, 1e-5, "losses vs oracle")
    assert_close(c.grad, c64.grad, 1e-4, "dc, all elements")
    assert_close(z.grad, z64.grad, 1e-4, "dz, all elements")
    for i in range(12):
        assert_close(crit.wPrediction.predictors[i].weight.grad, p64[f"wPrediction.predictors.{i}.weight"].grad, 2e-4, f"dW{i}, all elements")


@pytest.mark.parametrize("b,t_len,har,henc,k,nn", [(1, 14, 32, 32, 1, 1), (3, 20, 32, 64, 5, 3), (2, 40, 64, 32, 16, 17),
                                                   (5, 33, 128, 128, 7, 129), (2, 64, 32, 512, 12, 40), (9, 17, 24, 32, 3, 250),
                                                   # hidden 256 / 512: the streaming forward kernel and the one-kernel backward, every
                                                   # prediction-step count class (1-4, 5-8, 9-12, 13-16), few and many candidate tiles
                                                   (2, 24, 64, 256, 3, 16), (3, 30, 32, 256, 7, 48), (2, 40, 96, 256, 16, 32),
                                                   (1, 20, 32, 512, 1, 16), (2, 36, 64, 512, 14, 256), (2, 28, 32, 256, 12, 24)])
def test_criterion_odd_shapes_vs_oracle_fp64(b, t_len, har, henc, k, nn):
    """Shapes off every tile size of the criterion kernels (candidate tiles of 16 / 32, 16 prediction rows, lane groups):
    one window, one step, one negative, more negatives than a tile, all supported encoder widths -- vs the fp64 oracle."""
    crit = make_criterion(k, har, henc, nn, 200 + k, scale=3.0)
    cp = synth.predictor_params(k, har, henc, seed=200 + k, scale=3.0)
    c = synth.features((b, t_len, har), 201)
    z = synth.features((b, t_len, henc), 202, relu=True)
    cd, zd = c.to(DEV).requires_grad_(True), z.to(DEV).requires_grad_(True)
    crit.seed(77)
    losses, acc = crit(cd, zd, None)
    losses.sum().backward()
    p64 = {n: v.double().requires_grad_(True) for n, v in cp.items()}
    c64, z64 = c.double().requires_grad_(True), z.double().requires_grad_(True)
    _, _, ext = negative_indices(MT19937(77), b, t_len, t_len - k, nn)
    ref_losses, ref_acc = O.criterion_forward(c64, z64, O.predictor_list(p64, k), ext, nn)
    ref_losses.sum().backward()
    assert_close(losses, ref_losses, 1e-5, "losses")
    assert torch.allclose(acc.cpu().double(), ref_acc, atol=2.5 / (b * (t_len - k)))     # a float tie may flip an argmax
    assert_close(cd.grad, c64.grad, 1e-4, "dc")
    assert_close(zd.grad, z64.grad, 1e-4, "dz")
    for i in range(k):
        assert_close(crit.wPrediction.predictors[i].weight.grad, p64[f"wPrediction.predictors.{i}.weight"].grad, 2e-4, f"dW{i}")


@pytest.mark.parametrize("variant", ["skip", "reverse", "quality"])
@pytest.mark.parametrize("henc", [256, 512])
def test_criterion_variants_at_hidden_256_512_vs_oracle_fp64(variant, henc):
    """n_skipped, mode='reverse' and the signal-quality weights on the kernels that only hidden 256 / 512 use (the streaming
    forward kernel, the one-kernel backward); the reference-made goldens of these variants are at hidden 32."""
    b, t_len, har, k, nn = 3, 40, 64, 12, 32
    kw, okw = {}, {}
    if variant == "skip":
        kw["n_skipped"] = okw["n_skipped"] = 2
    if variant == "reverse":
        kw["mode"] = okw["mode"] = "reverse"
    if variant == "quality":
        kw.update(growth_rate=2.0, inflection_point_x=0.1)
    crit = make_criterion(k, har, henc, nn, 300, scale=3.0, **kw)
    cp = synth.predictor_params(k, har, henc, seed=300, scale=3.0)
    c = synth.features((b, t_len, har), 301)
    z = synth.features((b, t_len, henc), 302, relu=True)
    quality = torch.rand(b, 9, generator=torch.Generator().manual_seed(5)) if variant == "quality" else None
    if quality is not None:
        okw["weights"] = O.quality_weights(quality.double(), 2.0, 0.1, t_len - k)
    cd, zd = c.to(DEV).requires_grad_(True), z.to(DEV).requires_grad_(True)
    crit.seed(78)
    losses, acc = crit(cd, zd, None, None if quality is None else quality.to(DEV))
    losses.sum().backward()
    p64 = {n: v.double().requires_grad_(True) for n, v in cp.items()}
    c64, z64 = c.double().requires_grad_(True), z.double().requires_grad_(True)
    _, _, ext = negative_indices(MT19937(78), b, t_len, t_len - k, nn)
    ref_losses, ref_acc = O.criterion_forward(c64, z64, O.predictor_list(p64, k), ext, nn, **okw)
    ref_losses.sum().backward()
    assert losses.shape == ref_losses.shape
    assert_close(losses, ref_losses, 1e-5, "losses")
    assert torch.allclose(acc.cpu().double(), ref_acc, atol=2.5 / (b * (t_len - k)))
    assert_close(cd.grad, c64.grad, 1e-4, "dc")
    assert_close(zd.grad, z64.grad, 1e-4, "dz")
    for i in range(k):
        ref = p64[f"wPrediction.predictors.{i}.weight"].grad
        got = crit.wPrediction.predictors[i].weight.grad
        if ref is None or float(ref.abs().max()) == 0.0:
            assert got is None or float(got.abs().max()) == 0.0
        else:
            assert_close(got, ref, 2e-4, f"dW{i}")


def test_criterion_transformer_predictors_vs_reference_golden(golden):
    """rnnMode='transformer' (the fork's default predictors, criterion.py:136-143), eval mode."""
    g = golden("g8_criterion_transformer_pred.npz")
    b, t_len, h, k, nn, seed = (int(v) for v in g["cfg"])
    crit = cpc2_amd.CPCUnsupersivedCriterion(k, h, h, nn, rnnMode="transformer", sizeInputSeq=t_len)
    assert sorted(n for n, _ in crit.named_parameters()) == [str(x) for x in g["param_names"]]
    sd = crit.state_dict()
    for i in range(k):
        sd.update(synth.transformer_params(h, h, t_len - k, seed=80 + i, prefix=f"wPrediction.predictors.{i}.0."))
    crit.load_state_dict(sd)
    crit = crit.to(DEV).eval()
    c = synth.features((b, t_len, h), 90).to(DEV).requires_grad_(True)
    z = synth.features((b, t_len, h), 91, relu=True).to(DEV).requires_grad_(True)
    torch.manual_seed(seed)
    losses, acc = crit(c, z, None)
    assert_close(losses, t(g["losses"]), 1e-5, "losses")
    assert torch.allclose(acc.cpu(), t(g["acc"]), atol=1.5 / (b * (t_len - k)))
    losses.sum().backward()
    assert_close(c.grad, t(g["dc"]), 2e-4, "dc")
    assert_close(z.grad, t(g["dz"]), 1e-4, "dz")
    for name, prm in crit.named_parameters():
        if "grad." + name in g.files:
            assert_close(prm.grad, t(g["grad." + name]), 5e-4, f"grad {name}")


@pytest.mark.parametrize("mode,gates", [("LSTM", 4), ("RNN", 1)])
def test_criterion_recurrent_predictors_vs_reference_golden(golden, mode, gates):
    """rnnMode='LSTM' / 'RNN' (criterion.py:115-123): same state-dict keys, losses and gradients as the reference."""
    g = golden("g14_criterion_recurrent_pred.npz")
    b, t_len, har, henc, k, nn, seed = (int(v) for v in g["cfg"])
    crit = cpc2_amd.CPCUnsupersivedCriterion(k, har, henc, nn, rnnMode=mode, sizeInputSeq=t_len)
    sd = {}
    for i in range(k):
        sd.update(synth.gru_params(har, henc, 1, seed=110 + i, prefix=f"wPrediction.predictors.{i}.", gates=gates))
    assert sorted(sd) == sorted(crit.state_dict())
    crit.load_state_dict(sd)
    crit = crit.to(DEV)
    c = synth.features((b, t_len, har), 120).to(DEV).requires_grad_(True)
    z = synth.features((b, t_len, henc), 121, relu=True).to(DEV).requires_grad_(True)
    torch.manual_seed(seed)
    losses, acc = crit(c, z, None)
    assert_close(losses, t(g[f"{mode}_losses"]), 1e-5, "losses")
    assert torch.allclose(acc.cpu(), t(g[f"{mode}_acc"]), atol=1.5 / (b * (t_len - k)))
    losses.sum().backward()
    assert_close(c.grad, t(g[f"{mode}_dc"]), 2e-4, "dc")
    assert_close(z.grad, t(g[f"{mode}_dz"]), 1e-4, "dz")
    for name, prm in crit.named_parameters():
        assert_close(prm.grad, t(g[f"{mode}_grad." + name]), 5e-4, f"grad {name}")


def test_criterion_multihead_predictor_vs_reference_golden(golden):
    """--multihead_rnn with rnnMode='transformer' (criterion.py:44-94, transformers.py:137-158,190-212), eval mode."""
    g = golden("g9_criterion_multihead_pred.npz")
    b, t_len, h, k, nn, seed = (int(v) for v in g["cfg"])
    crit = cpc2_amd.CPCUnsupersivedCriterion(k, h, h, nn, rnnMode="transformer", sizeInputSeq=t_len, multihead_rnn=True)
    assert sorted(n for n, _ in crit.named_parameters()) == [str(x) for x in g["param_names"]]
    assert [str(tuple(v.shape)) for _, v in sorted(crit.state_dict().items())] == [str(x) for x in g["param_shapes"]]
    sd = crit.state_dict()
    sd.update(synth.transformer_params(h, h, t_len - k, seed=95, prefix="wPrediction.predictor.0.", n_classifiers=k))
    crit.load_state_dict(sd)
    crit = crit.to(DEV).eval()
    c = synth.features((b, t_len, h), 96).to(DEV).requires_grad_(True)
    z = synth.features((b, t_len, h), 97, relu=True).to(DEV).requires_grad_(True)
    torch.manual_seed(seed)
    losses, acc = crit(c, z, None)
    assert_close(losses, t(g["losses"]), 1e-5, "losses")
    assert torch.allclose(acc.cpu(), t(g["acc"]), atol=1.5 / (b * (t_len - k)))
    losses.sum().backward()
    assert_close(c.grad, t(g["dc"]), 2e-4, "dc")
    assert_close(z.grad, t(g["dz"]), 1e-4, "dz")
    for name, prm in crit.named_parameters():
        assert_close(prm.grad, t(g["grad." + name]), 5e-4, f"grad {name}")


def test_multiclassifier_head_vs_oracle_fp64():
    """MultiClassifierTransformerHead at the training shape family (12 classifiers, sizeSeq 116, H = 64)."""
    from cpc2_amd.transformers import buildMultHeadTransformerAR
    n, s, d, k = 2, 116, 64, 12
    net = buildMultHeadTransformerAR(d, d, 1, s, False, k)
    p = synth.transformer_params(d, d, s, seed=33, prefix="0.", n_classifiers=k)
    net.load_state_dict({**net.state_dict(), **p})
    net = net.to(DEV).eval()
    x = synth.features((n, s, d), 34)
    p64 = {kk: v.double().requires_grad_(True) for kk, v in p.items()}
    x64 = x.double().requires_grad_(True)
    ref = O.transformer_layer_forward(x64, p64, "0.", n_classifiers=k)
    gout = synth.features((n, s, k, d), 35)
    (ref * gout.double()).sum().backward()
    xd = x.to(DEV).requires_grad_(True)
    out = net(xd)
    assert out.shape == (n, s, k, d)
    assert_close(out, ref, 2e-5, "head out")
    (out * gout.to(DEV)).sum().backward()
    assert_close(xd.grad, x64.grad, 2e-4, "head dx")
    for name, prm in net.named_parameters():
        assert_close(prm.grad, p64[name].grad, 3e-4, f"head grad {name}")


def test_criterion_indices_on_device_are_bit_exact(golden):
    g = golden("g1_negidx.npz")
    seed, b, t_len, k, nn = (int(v) for v in g["mid_cfg"])
    crit = make_criterion(k, 32, 32, nn, 50)
    torch.manual_seed(seed)
    ext = crit.sampleIndices(b, t_len, t_len - k, torch.device(DEV), time_major=False)
    assert np.array_equal(ext.cpu().numpy().astype(np.int64), g["mid_extIdx"])
    torch.manual_seed(seed)                     # kernel layout: same values, [b, W, n_neg]
    ext_tm = crit.sampleIndices(b, t_len, t_len - k, torch.device(DEV)).cpu().numpy().astype(np.int64)
    assert np.array_equal(ext_tm.reshape(b, t_len - k, nn), g["mid_extIdx"].reshape(b, nn, t_len - k).transpose(0, 2, 1))


def test_device_index_expansion_on_ragged_shapes():
    """The device half of the sampler (raw words -> indices) against the host sampler on odd shapes, incl. one window,
    one negative, a window as long as the sequence minus one, and the large-config sizes."""
    rs = np.random.RandomState(3)
    shapes = [(1, 3, 1, 1), (2, 5, 4, 1), (7, 33, 20, 5), (3, 128, 127, 9), (64, 128, 116, 256)]
    shapes += [(int(rs.randint(1, 12)), int(t), int(rs.randint(1, t)), int(rs.randint(1, 40))) for t in rs.randint(3, 200, size=6)]
    for b, t_len, w, nn in shapes:
        host, dev = cpc2_amd.criterion.NegativeSampler(), cpc2_amd.criterion.NegativeSampler()
        host.seed(b * 1000 + w)
        dev.seed(b * 1000 + w)
        for _ in range(2):
            want = host.sample_host(b, t_len, w, nn, time_major=True)
            got = dev.sample(b, t_len, w, nn, torch.device(DEV)).cpu()
            assert torch.equal(got, want), (b, t_len, w, nn)
            assert int(got.min()) >= 0 and int(got.max()) < b * t_len


def test_device_index_expansion_and_prefetch_are_bit_exact():
    """host draw + device expansion == full host sampler; one-step-ahead prefetch leaves the stream unchanged."""
    b, t_len, k, nn = 8, 128, 12, 128
    ref = cpc2_amd.criterion.NegativeSampler()
    ref.seed(42)
    a = cpc2_amd.criterion.NegativeSampler()
    a.seed(42)
    p = cpc2_amd.criterion.NegativeSampler()
    p.seed(42)
    p.prefetch = True
    for _ in range(3):
        want = ref.sample_host(b, t_len, t_len - k, nn, time_major=True)
        assert torch.equal(a.sample(b, t_len, t_len - k, nn, torch.device(DEV)).cpu(), want)
        assert torch.equal(p.sample(b, t_len, t_len - k, nn, torch.device(DEV)).cpu(), want)


_FULL_BATCH_ORACLE = {}


def _full_batch_criterion_case(h, nn):
    """Inputs and the sparse fp64 oracle's outputs of the criterion at b = 64 (C2: the very case of golden g18; C5 per GPU)."""
    if (h, nn) not in _FULL_BATCH_ORACLE:
        b, t_len, k, seed, pseed = 64, 128, 12, 4321, 160
        cp = synth.predictor_params(k, h, h, seed=pseed, scale=2.0)              # trained-scale predictors
        c = synth.features((b, t_len, h), pseed + 1)
        z = synth.features((b, t_len, h), pseed + 2, relu=True)
        _, _, ext = negative_indices(MT19937(seed), b, t_len, t_len - k, nn)
        dl = torch.linspace(0.5, 1.5, k, dtype=torch.float64)
        ones = O.criterion_forward_sparse(c.double(), z.double(), O.predictor_list({n: v.double() for n, v in cp.items()}, k), ext, nn)
        ramp = O.criterion_forward_sparse(c.double(), z.double(), O.predictor_list({n: v.double() for n, v in cp.items()}, k), ext, nn,
                                          dlosses=dl)
        ext_tm = torch.as_tensor(np.asarray(ext).reshape(b, nn, t_len - k).transpose(0, 2, 1).copy(), dtype=torch.int32)
        _FULL_BATCH_ORACLE[(h, nn)] = (cp, c, z, ext_tm, dl, ones, ramp)
    return _FULL_BATCH_ORACLE[(h, nn)]


@pytest.mark.parametrize("h,nn", [(256, 128), (512, 256)])
def test_criterion_at_full_batch_vs_oracle_module_call(golden, h, nn):
    """The criterion's kernels at the launch geometry of the benchmark -- b = 64: 7 424 (b,t) items, 950 272 / 1 900 544
    references in the counting-sorted dz lists, 8 192 z rows -- against the sparse fp64 oracle, EVERY element of every gradient
    (criterion.py:237-286, 329-363); predictors at trained scale, so a wrong gather row or a dropped reference shows.  At C2 the
    oracle is itself pinned to the reference's own b = 64 run (g18, tests/test_oracle_golden.py) and the kernels are compared with
    that golden directly as well.  This is the module call: the immediate backward, T context frames, indices from the sampler."""
    cp, c, z, _ext, _dl, ref, _ = _full_batch_criterion_case(h, nn)
    b, t_len, k = 64, 128, 12
    crit = cpc2_amd.CPCUnsupersivedCriterion(k, h, h, nn, rnnMode="linear", sizeInputSeq=t_len)
    crit.load_state_dict(cp)
    crit = crit.to(DEV)
    cd, zd = c.to(DEV).requires_grad_(True), z.to(DEV).requires_grad_(True)
    torch.manual_seed(4321)                     # the reference drew its negatives from this CPU stream
    losses, acc = crit(cd, zd, None)
    losses.sum().backward()
    assert_close(losses, ref["losses"], 1e-5, "losses")
    assert torch.allclose(acc.cpu().double(), ref["acc"], atol=2.5 / (b * (t_len - k)))
    assert_close(cd.grad, ref["dc"], 1e-4, "dc, all elements")
    assert_close(zd.grad, ref["dz"], 1e-4, "dz, all elements")
    for i in range(k):
        assert_close(crit.wPrediction.predictors[i].weight.grad, ref["dW"][i], 2e-4, f"dW{i}, all elements")
    if (h, nn) == (256, 128):
        g = golden("g18_criterion_b64.npz")
        assert_close(losses, t(g["losses"]), 1e-5, "losses vs the reference's b = 64 run")
        assert_close(zd.grad[::9, ::5, ::37], t(g["dz_sample"]), 1e-4, "dz sample vs reference")
        assert_close(cd.grad[::9, ::5, ::37], t(g["dc_sample"]), 1e-4, "dc sample vs reference")
        assert_close(zd.grad[:, -14:, :8], t(g["dz_tail"]), 1e-4, "dz tail vs reference")
        for i in range(k):
            assert_close(crit.wPrediction.predictors[i].weight.grad[::17, ::13], t(g[f"dW{i}_sample"]), 2e-4, f"dW{i} sample vs reference")


@pytest.mark.parametrize("deferred", [0, 1])
@pytest.mark.parametrize("h,nn", [(256, 128), (512, 256)])
def test_criterion_at_full_batch_vs_oracle_step_form(h, nn, deferred):
    """The form cpcStep runs (cpc_infonce_forward / backward with c_frames = W: the context handed over as its W frames; deferred = 1: dz and
    the predictor gradients on the library's side stream, joined afterwards) at b = 64 against the sparse fp64 oracle, with a
    non-uniform gradient of the losses."""
    lib = _lib.load()
    cp, c, z, ext_tm, dl, _, ref = _full_batch_criterion_case(h, nn)
    b, t_len, k = 64, 128, 12
    w_len = t_len - k
    cw = c[:, :w_len].contiguous().to(DEV)
    zd, ext = z.to(DEV), ext_tm.to(DEV)
    wpred = torch.stack([cp[f"wPrediction.predictors.{i}.weight"] for i in range(k)]).to(DEV)
    dld = dl.float().to(DEV)
    st = _lib.stream_ptr(cw.device)
    saved = torch.empty(lib.cpc_infonce_saved_bytes(b, t_len, k, h, h, nn), dtype=torch.uint8, device=DEV)
    scr = torch.empty(lib.cpc_infonce_scratch_bytes(b, t_len, k, h, h, nn), dtype=torch.uint8, device=DEV)
    losses, acc = torch.empty(k, device=DEV), torch.empty(k, device=DEV)
    _lib.check(lib.cpc_infonce_forward(_lib.ptr(cw), _lib.ptr(zd), _lib.ptr(wpred), _lib.ptr(ext), None, _lib.ptr(losses), _lib.ptr(acc),
                                       _lib.ptr(saved), _lib.ptr(scr), b, t_len, w_len, k, h, h, nn, st), "fwd")
    dc, dz, dw = torch.full_like(cw, float("nan")), torch.full_like(zd, float("nan")), torch.full_like(wpred, float("nan"))
    _lib.check(lib.cpc_infonce_backward(_lib.ptr(cw), _lib.ptr(zd), _lib.ptr(wpred), _lib.ptr(ext), None, _lib.ptr(dld), _lib.ptr(saved),
                                        _lib.ptr(scr), _lib.ptr(dc), _lib.ptr(dz), _lib.ptr(dw), b, t_len, w_len, k, h, h, nn, deferred, st), "bwd")
    if deferred:
        _lib.check(lib.cpc_infonce_join(st), "join")
    torch.cuda.synchronize()
    _lib.check(lib.cpc_async_error_check(st), "async errors")
    assert_close(losses.view(1, -1), ref["losses"], 1e-5, "losses")
    assert torch.allclose(acc.cpu().double().view(1, -1), ref["acc"], atol=2.5 / (b * w_len))
    assert_close(dc, ref["dc"][:, :w_len], 1e-4, "dc, all elements")
    assert_close(dz, ref["dz"], 1e-4, "dz, all elements")
    for i in range(k):
        assert_close(dw[i], ref["dW"][i], 2e-4, f"dW{i}, all elements")


@pytest.mark.parametrize("h,nn", [(256, 128), (512, 256)])
def test_criterion_properties_at_full_size(h, nn):
    """b=64 (BASELINE configs C2 and, hidden 512 / 256 negatives, C5 per GPU): untrained-predictor loss is ln(1+Nneg) for every
    step; the loss does not depend on a common shift of all logits; gradients are finite and dz rows beyond reach are zero."""
    b, t_len, k = 64, 128, 12
    crit = make_criterion(k, h, h, nn, 70, scale=0.0)            # zero predictors -> uniform logits
    c = synth.features((b, t_len, h), 71).to(DEV).requires_grad_(True)
    z = synth.features((b, t_len, h), 72, relu=True).to(DEV).requires_grad_(True)
    crit.seed(5)
    losses, acc = crit(c, z, None)
    assert torch.allclose(losses.cpu(), torch.full((1, k), float(np.log(nn + 1))), atol=1e-5)
    assert torch.allclose(acc.cpu(), torch.ones(1, k))          # all ties -> index 0 wins (criterion.py:356)
    crit2 = make_criterion(k, h, h, nn, 73, scale=2.0)
    crit2.seed(5)
    l2, _ = crit2(c, z, None)
    l2.sum().backward()
    assert torch.isfinite(c.grad).all() and torch.isfinite(z.grad).all()
    assert float(c.grad[:, t_len - k:].abs().max()) == 0.0       # context frames >= W are never used
    # two identical calls with the same index stream: same losses, and the SAME dz bit for bit -- the contributions
    # of the negatives are summed per z row from sorted reference lists, not with atomics
    dz_first = z.grad.clone()
    z.grad = None
    crit2.seed(5)
    l3, _ = crit2(c, z, None)
    assert torch.equal(l2, l3)
    l3.sum().backward()
    assert torch.equal(z.grad, dz_first)


def test_model_span_masking_vs_reference_golden(golden):
    """CPCModel(mask_prob > 0) (model.py:300-390), forward (the reference's own backward fails: it writes in place into
    the ReLU output autograd needs); here the masked frames simply get no encoder gradient and mask_emb gets theirs."""
    g = golden("g11_model_span_mask.npz")
    hidden, n = (int(v) for v in g["cfg"])
    mp = synth.encoder_params(hidden, 11)
    mp.update(synth.gru_params(hidden, hidden, 1, 41))
    model = cpc2_amd.CPCModel(cpc2_amd.CPCEncoder(hidden), cpc2_amd.CPCAR(hidden, hidden, False, 1), mask_prob=0.02, mask_length=4)
    mp["mask_emb"] = t(g["mask_emb"])
    model.load_state_dict(mp)
    model = model.to(DEV)
    x = synth.audio_windows(n, 20480, 12).to(DEV)
    np.random.seed(5)
    c, z, _ = model(x, None)
    assert_close(z, t(g["z"]), 2e-5, "masked encodedData")
    assert_close(c, t(g["c"]), 2e-5, "context")
    masked = (z == model.mask_emb).all(dim=2)
    assert 0 < int(masked.sum()) < n * 128
    (c.sum() + z.sum()).backward()
    assert torch.isfinite(model.mask_emb.grad).all() and float(model.mask_emb.grad.abs().sum()) > 0
    assert torch.isfinite(model.gEncoder.conv0.weight.grad).all()


# ----------------------------------------------------------------------------- transformer AR (config 4)
def load_transformer(d_model, d_out, size_seq, params, n_layers=1):
    from cpc2_amd.transformers import buildTransformerAR
    net = buildTransformerAR(d_out, d_model, n_layers, size_seq, False)
    sd = {k[len("gAR."):]: v for k, v in params.items()}
    sd.update({k: v for k, v in net.state_dict().items() if k.endswith(".z") or k.endswith(".mask")})
    net.load_state_dict(sd)
    return net.to(DEV)


def test_transformer_vs_reference_golden(golden):
    g = golden("g7_transformer.npz")
    d_model, s, n = (int(v) for v in g["cfg"])
    net = load_transformer(d_model, d_model, s, synth.transformer_params(d_model, d_model, s, 71)).eval()
    x = synth.features((n, s, d_model), 72, relu=True).to(DEV).requires_grad_(True)
    out = net(x)
    assert_close(out, t(g["out"]), 2e-5, "transformer out")
    (out * synth.features((n, s, d_model), 73).to(DEV)).sum().backward()
    assert_close(x.grad, t(g["dx"]), 1e-4, "transformer dx")
    for name, p in net.named_parameters():
        assert_close(p.grad, t(g["grad." + name]), 2e-4, f"transformer grad {name}")


# d_model 256 (head size 32) takes the MFMA attention kernels: full 128-frame window, the predictors' 116 frames (ragged
# last tile), 32-frame blocks of a longer input, 40 frames (two waves idle)
@pytest.mark.parametrize("tag", ["abspos", "ragged", "abspos_ragged"])
def test_transformer_variants_vs_reference_golden(golden, tag):
    """abspos=True (StaticPositionEmbedding in front, no Krelpos) and lengths that are not a multiple of sizeSeq
    (zero-padded blocks, transformers.py:38-50)."""
    from cpc2_amd.transformers import buildTransformerAR
    g = golden("g10_transformer_variants.npz")
    d_model, size_seq, n = (int(v) for v in g["cfg"])
    s_len = int(g[tag + "_len"])
    abspos = tag.startswith("abspos")
    net = buildTransformerAR(d_model, d_model, 1, size_seq, abspos)
    assert sorted(net.state_dict().keys()) == [str(x) for x in g[tag + "_keys"]]
    layer = "1." if abspos else "0."
    p = synth.transformer_params(d_model, d_model, size_seq, 171)
    sd = {layer + k[len("gAR.0."):]: v for k, v in p.items() if not (abspos and k.endswith("Krelpos"))}
    net.load_state_dict({**net.state_dict(), **sd})
    net = net.to(DEV).eval()
    x = synth.features((n, s_len, d_model), 172, relu=True).to(DEV).requires_grad_(True)
    out = net(x)
    assert_close(out, t(g[tag + "_out"]), 2e-5, "out")
    (out * synth.features((n, s_len, d_model), 173).to(DEV)).sum().backward()
    assert_close(x.grad, t(g[tag + "_dx"]), 1e-4, "dx")
    for name, prm in net.named_parameters():
        assert_close(prm.grad, t(g[tag + "_grad." + name]), 2e-4, f"grad {name}")


@pytest.mark.parametrize("d_model,size_seq,s,n", [(256, 128, 128, 3), (64, 32, 96, 2), (512, 128, 128, 1), (256, 116, 116, 2),
                                                    (256, 32, 96, 2), (256, 40, 40, 3)])
def test_transformer_vs_oracle_fp64(d_model, size_seq, s, n):
    params = synth.transformer_params(d_model, d_model, size_seq, 81)
    net = load_transformer(d_model, d_model, size_seq, params).eval()
    x = synth.features((n, s, d_model), 82, relu=True)
    p64 = {k: v.double().requires_grad_(True) for k, v in params.items()}
    x64 = x.double().requires_grad_(True)
    # sequences longer than sizeSeq are attended in independent blocks (transformers.py:38-50)
    ref = O.transformer_layer_forward(x64.view(n * (s // size_seq), size_seq, d_model), p64, "gAR.0.").view(n, s, d_model)
    gout = synth.features((n, s, d_model), 83)
    (ref * gout.double()).sum().backward()
    xd = x.to(DEV).requires_grad_(True)
    out = net(xd)
    assert_close(out, ref, 2e-5, "transformer out")
    (out * gout.to(DEV)).sum().backward()
    assert_close(xd.grad, x64.grad, 1e-4, "transformer dx")
    for name, p in net.named_parameters():
        assert_close(p.grad, p64["gAR." + name].grad, 2e-4, f"transformer grad {name}")


def test_transformer_dropout_training_mode():
    """p = 0.1 in training mode: masks come from a hash (not torch's stream); properties only -- deterministic for a fixed
    seed, different from eval, finite gradients.  The values are held to the fp64 oracle under the rebuilt masks by
    tests/test_transformer_dropout_gpu.py."""
    params = synth.transformer_params(64, 64, 32, 91)
    net = load_transformer(64, 64, 32, params)
    x = synth.features((4, 32, 64), 92, relu=True).to(DEV).requires_grad_(True)
    net.eval()
    ref = net(x).detach()
    net.train()
    torch.manual_seed(5)
    a = net(x)
    torch.manual_seed(5)
    b = net(x)
    assert torch.allclose(a, b, atol=1e-5, rtol=1e-5)     # same masks (K splits are reduced in a fixed order: no atomics)
    assert not torch.allclose(a, ref, atol=1e-4)
    a.sum().backward()
    assert torch.isfinite(x.grad).all()
    assert all(torch.isfinite(p.grad).all() for p in net.parameters())


def test_transformer_dropout_gradient_is_consistent_at_head_size_32():
    """d_model 256 (MFMA attention), p = 0.1: forward and backward must draw the same masks -- checked with a
    directional finite difference of sum(out * g) along a random direction in x (fp32: loose tolerance)."""
    params = synth.transformer_params(256, 256, 116, 93)
    net = load_transformer(256, 256, 116, params).train()
    x = synth.features((2, 116, 256), 94, relu=True).to(DEV)
    g = synth.features((2, 116, 256), 95).to(DEV)
    v = synth.features((2, 116, 256), 96).to(DEV)

    def f(inp):
        torch.manual_seed(11)                  # same dropout seed every call
        return (net(inp) * g).sum()
    xr = x.clone().requires_grad_(True)
    f(xr).backward()
    analytic = float((xr.grad * v).sum())
    eps = 1e-2
    with torch.no_grad():
        numeric = float((f(x + eps * v).double() - f(x - eps * v).double()) / (2 * eps))
    assert abs(analytic - numeric) <= 2e-2 * max(1.0, abs(numeric)), (analytic, numeric)


@pytest.mark.parametrize("hidden,nn", [(64, 16), (256, 128)])
def test_model_with_transformer_ar_train_step_vs_oracle(hidden, nn):
    """One full step with arMode='transformer' (feature_loader.py:216-220, transformers.py:119-134): loss and EVERY gradient
    against the fp64 oracle.  (256, 128) is BASELINE configs[3] at its real shapes -- d_model 256 = head size 32: the MFMA
    attention kernels, the plane-fed encoder GEMMs, the LDS-DMA InfoNCE kernels -- at b = 2."""
    b, k = 2, 12
    mp = synth.encoder_params(hidden, 21)
    mp.update(synth.transformer_params(hidden, hidden, 128, 25))
    from cpc2_amd.transformers import buildTransformerAR
    ar = buildTransformerAR(hidden, hidden, 1, 128, False)
    model = cpc2_amd.CPCModel(cpc2_amd.CPCEncoder(hidden), ar)
    sd = dict(mp)
    sd.update({kk: v for kk, v in model.state_dict().items() if kk.endswith(".z") or kk.endswith(".mask")})
    model.load_state_dict(sd)
    crit = cpc2_amd.CPCUnsupersivedCriterion(k, hidden, hidden, nn, rnnMode="linear", sizeInputSeq=128)
    cp = synth.predictor_params(k, hidden, hidden, 23)
    crit.load_state_dict(cp)
    model, crit = model.to(DEV).eval(), crit.to(DEV)          # eval: dropout off (parity is defined at p = 0)
    x = synth.audio_windows(b, 20480, 24)
    crit.seed(77)
    tot, losses, _ = cpcStep(x.to(DEV), x.to(DEV), torch.zeros(b, dtype=torch.long, device=DEV), model, crit)
    tot.backward()
    p64 = {kk: v.double().requires_grad_(True) for kk, v in list(mp.items()) + list(cp.items())}
    ref_tot, ref_losses, _ = O.train_step_loss(x.double(), x.double(), {kk: p64[kk] for kk in mp}, {kk: p64[kk] for kk in cp},
                                               MT19937(77), k, nn, 1, ar="transformer")
    ref_tot.backward()
    assert_close(losses, ref_losses, 1e-5, "losses")
    for name, p in list(model.named_parameters()) + list(crit.named_parameters()):
        assert_close(p.grad, p64[name].grad, 5e-4, f"grad {name}")


@pytest.mark.parametrize("mode,layers", [("LSTM", 2), ("RNN", 1)])
def test_model_with_lstm_ar_train_step_vs_oracle(mode, layers):
    """The fork's default model (arMode='LSTM', cpc_default_config.py) through one full step: loss and every gradient."""
    hidden, b, k, nn = 64, 2, 12, 16
    mp = synth.encoder_params(hidden, 21)
    mp.update(_RECURRENT[mode][0](hidden, hidden, layers, 26))
    model = cpc2_amd.CPCModel(cpc2_amd.CPCEncoder(hidden), cpc2_amd.CPCAR(hidden, hidden, False, layers, mode=mode))
    model.load_state_dict(mp)
    crit = cpc2_amd.CPCUnsupersivedCriterion(k, hidden, hidden, nn, rnnMode="linear", sizeInputSeq=128)
    cp = synth.predictor_params(k, hidden, hidden, 23)
    crit.load_state_dict(cp)
    model, crit = model.to(DEV), crit.to(DEV)
    x = synth.audio_windows(b, 20480, 24)
    crit.seed(78)
    tot, losses, _ = cpcStep(x.to(DEV), x.to(DEV), torch.zeros(b, dtype=torch.long, device=DEV), model, crit)
    tot.backward()
    p64 = {kk: v.double().requires_grad_(True) for kk, v in list(mp.items()) + list(cp.items())}
    ref_tot, ref_losses, _ = O.train_step_loss(x.double(), x.double(), {kk: p64[kk] for kk in mp}, {kk: p64[kk] for kk in cp},
                                               MT19937(78), k, nn, layers, ar=mode)
    ref_tot.backward()
    assert_close(losses, ref_losses, 1e-5, "losses")
    for name, p in list(model.named_parameters()) + list(crit.named_parameters()):
        assert_close(p.grad, p64[name].grad, 5e-4, f"grad {name}")


# ----------------------------------------------------------------------------- Adam + full train steps
def test_fused_adam_vs_oracle():
    g = torch.Generator().manual_seed(0)
    p0 = {"a": torch.randn(1000, generator=g), "b": torch.randn(33, 7, generator=g)}
    prm = [torch.nn.Parameter(v.clone().to(DEV)) for v in p0.values()]
    opt = FlatAdam(prm, lr=2e-4)
    ref = O.Adam({k: v.clone().double() for k, v in p0.items()}, lr=2e-4)
    for step in range(5):
        grads = {k: torch.randn(v.shape, generator=g) for k, v in p0.items()}
        for p, gr in zip(prm, grads.values()):
            p.grad = gr.to(DEV)              # a gradient produced outside the fused kernels: gathered by step()
        opt.step()
        opt.zero_grad()
        ref.step({k: v.double() for k, v in grads.items()})
    for p, r in zip(prm, ref.params.values()):
        assert_close(p.data, r, 1e-6, "adam params")


def test_flat_adam_is_a_torch_optimizer_the_schedulers_drive():
    """train.py:501-520: the reference's StepLR / ramp / SchedulerCombiner attach to the optimiser and the fused update
    uses the scheduled rate (zero gradient history: the first Adam step moves every weight by exactly lr)."""
    import warnings
    from cpc2_amd.train import buildScheduler
    w = torch.nn.Parameter(torch.zeros(1000, device=DEV))
    opt = FlatAdam([w], lr=2e-4)
    assert isinstance(opt, torch.optim.Optimizer)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sched = buildScheduler(opt, 3, 4, 0)
    ref = np.load(os.path.join(os.path.dirname(__file__), "golden", "g13_lr_schedules.npz"))["ramp4_step3"]
    for epoch in range(8):
        lr = opt.param_groups[0]["lr"]
        assert abs(lr - ref[epoch]) <= 1e-12 * ref[epoch]
        if epoch == 0:
            w.grad = None
            before = w.detach().clone()
            (w.sum()).backward()
            opt.step()
            opt.zero_grad()
            assert_close(before - w.detach(), torch.full((1000,), float(lr)), 1e-5, "first Adam step = lr")
        else:
            opt.step()
        sched.step()


def test_dedup_step_matches_reference_semantics():
    hidden, b, k, nn = 64, 3, 12, 16
    mp = synth.encoder_params(hidden, 21)
    mp.update(synth.gru_params(hidden, hidden, 1, 22))
    model = cpc2_amd.CPCModel(cpc2_amd.CPCEncoder(hidden), cpc2_amd.CPCAR(hidden, hidden, False, 1))
    model.load_state_dict(mp)
    crit = cpc2_amd.CPCUnsupersivedCriterion(k, hidden, hidden, nn, rnnMode="linear", sizeInputSeq=128)
    crit.load_state_dict(synth.predictor_params(k, hidden, hidden, 23))
    model, crit = model.to(DEV), crit.to(DEV)
    x = synth.audio_windows(b, 20480, 24).to(DEV)
    label = torch.zeros(b, dtype=torch.long, device=DEV)
    outs = []
    for dedup in (False, True):
        crit.seed(3)
        model.zero_grad()
        tot, losses, acc = cpcStep(x, x, label, model, crit, dedup=dedup)
        tot.backward()
        outs.append((losses.detach().clone(), acc.clone(), model.gEncoder.conv1.weight.grad.clone()))
    # same arithmetic per window; only the summation order may differ (split-K choice depends on the row count,
    # weight gradients sum one pass instead of two halves)
    assert_close(outs[1][0], outs[0][0], 2e-6, "losses")
    assert torch.equal(outs[0][1], outs[1][1])
    assert_close(outs[1][2], outs[0][2], 2e-5, "conv1 grad")


def test_train_steps_reproduce_reference_loss_curve(golden):
    """G6: 20 Adam steps, H=64, b=4, reference semantics (model on cat([past, future]))."""
    g = golden("g6_trainsteps.npz")
    hidden, b, k, nn, steps, seed = (int(v) for v in g["cfg"])
    mp = synth.encoder_params(hidden, 21)
    mp.update(synth.gru_params(hidden, hidden, 1, 22))
    model = cpc2_amd.CPCModel(cpc2_amd.CPCEncoder(hidden), cpc2_amd.CPCAR(hidden, hidden, False, 1))
    model.load_state_dict(mp)
    crit = cpc2_amd.CPCUnsupersivedCriterion(k, hidden, hidden, nn, rnnMode="linear", sizeInputSeq=128)
    crit.load_state_dict(synth.predictor_params(k, hidden, hidden, 23))
    model, crit = model.to(DEV), crit.to(DEV)
    opt = buildOptimizer(model, crit, lr=2e-4)
    x = synth.audio_windows(b, 20480, 24).to(DEV)
    label = torch.zeros(b, dtype=torch.long, device=DEV)
    torch.manual_seed(seed)
    curve = []
    for _ in range(steps):
        tot, losses, _acc = cpcStep(x, x, label, model, crit)
        tot.backward()
        opt.step()
        opt.zero_grad()
        curve.append(losses.detach())
    curve = torch.cat(curve).cpu()
    ref = t(g["curve"])
    err = ((curve - ref).abs() / ref.abs()).max()
    assert err <= 1e-3, f"loss curve deviates by {float(err):.2e} relative"
    # Adam moves every weight by ~lr per step whatever the gradient's size, so weights whose gradient is
    # fp32 noise may end anywhere within steps*lr = 4e-3; the UPDATE as a whole must point the same way.
    init = mp["gEncoder.conv0.weight"]
    got, ref_w = model.state_dict()["gEncoder.conv0.weight"].cpu(), t(g["final.gEncoder.conv0.weight"])
    assert float((got - ref_w).abs().max()) <= steps * 2e-4 * 1.05
    d_got, d_ref = (got - init).flatten().double(), (ref_w - init).flatten().double()
    cos = float(d_got @ d_ref / (d_got.norm() * d_ref.norm()))
    assert cos >= 0.98, f"update direction cos {cos:.4f}"


# ----------------------------------------------------------------------------- feeder / features / checkpoints
GOLD_DB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test_db")
SEQ_LIST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seq_list.txt")


def _feeder(device, **kw):
    from cpc2_amd.dataset import AudioBatchData, filterSeqs, findAllSeqs
    seq_names, speakers = findAllSeqs(GOLD_DB, extension=".flac")
    seq_names = filterSeqs(SEQ_LIST, seq_names)
    return AudioBatchData(GOLD_DB, 20480, seq_names, None, len(speakers), device=device, **kw)


def test_feeder_windows_on_device_match_host_slices():
    import random
    random.seed(0)
    dev_data = _feeder(DEV)
    random.seed(0)
    cpu_data = _feeder("cpu")
    assert torch.equal(dev_data.data.cpu(), cpu_data.data)
    offs = [0, 1, 20479, 123457, cpu_data.data.numel() - 20480]
    assert torch.equal(dev_data.windows(offs).cpu(), cpu_data.windows(offs))
    torch.manual_seed(3)
    random.seed(3)
    batches = list(dev_data.getDataLoader(8, "uniform", True))
    assert len(batches) >= 5 and all(s.is_cuda and s.shape == (8, 2, 1, 20480) for s, _ in batches)
    # the device loader (a pack's offsets uploaded once, speaker labels looked up on the device) yields what the host loader
    # yields, batch for batch -- windows AND labels, ragged last batches of a speaker included (dataset.py:300-330)
    for kind in ("samespeaker", "samesequence", "temporalsamespeaker", "sequential"):
        torch.manual_seed(5)
        random.seed(5)
        on_dev = list(dev_data.getDataLoader(8, kind, True))
        torch.manual_seed(5)
        random.seed(5)
        on_cpu = list(cpu_data.getDataLoader(8, kind, True))
        assert len(on_dev) == len(on_cpu) > 0, kind
        for (sd, ld), (sc, lc) in zip(on_dev, on_cpu):
            assert torch.equal(sd.cpu(), sc) and torch.equal(ld.cpu(), lc), kind


def _small_model(hidden=64):
    mp = synth.encoder_params(hidden, 21)
    mp.update(synth.gru_params(hidden, hidden, 1, 22))
    model = cpc2_amd.CPCModel(cpc2_amd.CPCEncoder(hidden), cpc2_amd.CPCAR(hidden, hidden, False, 1))
    model.load_state_dict(mp)
    return model.to(DEV), mp


def test_build_feature_on_real_audio_vs_oracle():
    from cpc2_amd import audio
    from cpc2_amd.feature_loader import FeatureModule, buildFeature
    model, mp = _small_model()
    path = os.path.join(GOLD_DB, "4397", "15668", "4397-15668-0003.flac")
    wav = audio.load(path)[0]
    p64 = to64(mp)
    for get_encoded in (False, True):
        fm = FeatureModule(model, get_encoded).eval()
        feats = buildFeature(fm, path, maxSizeSeq=64000)
        ref = []
        for start in range(0, wav.shape[1], 64000):
            c, z = O.model_forward(wav[:, start:start + 64000].double().view(1, 1, -1), p64)
            ref.append(z if get_encoded else c)
        ref = torch.cat(ref, dim=1)
        assert feats.shape == ref.shape == (1, 400 + 400 + 359, 64)
        assert_close(feats, ref, 5e-5, f"features get_encoded={get_encoded}")
    strict = buildFeature(FeatureModule(model, False).eval(), path, strict=True, maxSizeSeq=64000)
    # two whole chunks, then the last 64 000 samples of which the frames the rest covers are kept
    assert wav.shape[1] // 64000 == 2 and (wav.shape[1] % 64000) // 160 == 359
    assert strict.shape == (1, 400 + 400 + 359, 64)


def test_checkpoint_roundtrip_in_reference_layout(tmp_path):
    from cpc2_amd.feature_loader import getCheckpointData, loadModel, save_checkpoint
    import json
    model, _ = _small_model()
    crit = cpc2_amd.CPCUnsupersivedCriterion(12, 64, 64, 16, rnnMode="linear", sizeInputSeq=128).to(DEV)
    opt = buildOptimizer(model, crit)
    x = synth.audio_windows(2, 20480, 24).to(DEV)
    crit.seed(1)
    tot, _, _ = cpcStep(x, x, torch.zeros(2, dtype=torch.long, device=DEV), model, crit)
    tot.backward()
    opt.step()
    opt.zero_grad()
    args = dict(hiddenEncoder=64, hiddenGar=64, normMode="layerNorm", arMode="GRU", samplingType="samespeaker",
                nLevelsGRU=1, cpc_mode=None, sizeWindow=20480, abspos=False, encoder_type="cpc")
    (tmp_path / "checkpoint_args.json").write_text(json.dumps(args))
    (tmp_path / "checkpoint_logs.json").write_text(json.dumps({"epoch": [0]}))
    path = str(tmp_path / "checkpoint_0.pt")
    save_checkpoint(model.state_dict(), crit.state_dict(), opt.state_dict(), model.state_dict(), path)
    blob = torch.load(path, "cpu")
    assert set(blob) == {"gEncoder", "cpcCriterion", "optimizer", "best"}
    assert "gEncoder.conv0.weight" in blob["gEncoder"] and "wPrediction.predictors.11.weight" in blob["cpcCriterion"]
    assert set(blob["optimizer"]["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    found, logs, loc_args = getCheckpointData(str(tmp_path))
    assert os.path.basename(found) == "checkpoint_0.pt" and loc_args.hiddenGar == 64
    model2, hg, he = loadModel([path])
    model2 = model2.to(DEV)
    assert (hg, he) == (64, 64)
    c1, z1, _ = model(x, None)
    c2, z2, _ = model2(x, None)
    assert_close(c2, c1, 1e-5, "c after reload")       # (every K split is reduced in a fixed order; the bound is just generous)
    assert_close(z2, z1, 1e-5, "z after reload")
    crit2 = cpc2_amd.CPCUnsupersivedCriterion(12, 64, 64, 16, rnnMode="linear", sizeInputSeq=128)
    crit2.load_state_dict(blob["cpcCriterion"])
    opt2 = buildOptimizer(model2, crit2.to(DEV))
    opt2.load_state_dict(blob["optimizer"])
    assert opt2.step_count == 1 and torch.equal(opt2.exp_avg, opt.exp_avg)


def test_training_steps_on_reference_test_data_vs_oracle():
    """BASELINE config C1 in miniature: real LibriSpeech windows from the reference's cpc/test_data fixture,
    sequential sampler (deterministic), 3 Adam steps; HIP loss curve vs the CPU oracle's."""
    import random
    hidden, b, k, nn, steps = 64, 4, 12, 32, 3
    model, mp = _small_model(hidden)
    cp = synth.predictor_params(k, hidden, hidden, 23)
    crit = cpc2_amd.CPCUnsupersivedCriterion(k, hidden, hidden, nn, rnnMode="linear", sizeInputSeq=128)
    crit.load_state_dict(cp)
    crit = crit.to(DEV)
    opt = buildOptimizer(model, crit, lr=2e-4)
    random.seed(0)
    data = _feeder(DEV)
    loader = iter(data.getDataLoader(b, "sequential", False))
    batches = [next(loader) for _ in range(steps)]
    crit.seed(99)
    curve = []
    for seq, label in batches:
        tot, losses, _ = cpcStep(seq[:, 0], seq[:, 1], label, model, crit, dedup=True)
        tot.backward()
        opt.step()
        opt.zero_grad()
        curve.append(losses.detach().cpu())
    # oracle on the same windows
    params = {n: v.clone().requires_grad_(True) for n, v in list(cp.items()) + list(mp.items())}
    adam = O.Adam({n: v.data for n, v in params.items()}, lr=2e-4)
    mt = MT19937(99)
    for step, (seq, _label) in enumerate(batches):
        xw = seq[:, 0].cpu()
        tot, losses, _ = O.train_step_loss(xw, xw, {n: params[n] for n in mp}, {n: params[n] for n in cp}, mt, k, nn)
        grads = torch.autograd.grad(tot, list(params.values()))
        adam.step(dict(zip(params, grads)))
        err = float(((curve[step] - losses.detach()).abs() / losses.detach().abs()).max())
        assert err <= 1e-3, f"step {step}: loss differs by {err:.2e}"


def test_run_epoch_loop_checkpoints_and_resumes(tmp_path):
    """train.py:190-255 on the reference's cpc/test_data fixture: two epochs with a ramp + step schedule, logs grow key by
    key, checkpoints in the reference layout every saveStep epochs; a second call resumes from len(logs["epoch"])."""
    import json
    import random
    from cpc2_amd.feature_loader import getCheckpointData, loadModel
    from cpc2_amd.train import buildScheduler, run
    hidden = 64
    model, _ = _small_model(hidden)
    crit = cpc2_amd.CPCUnsupersivedCriterion(12, hidden, hidden, 32, rnnMode="linear", sizeInputSeq=128).to(DEV)
    crit.seed(7)
    opt = buildOptimizer(model, crit, lr=2e-4)
    sched = buildScheduler(opt, schedulerStep=2, schedulerRamp=2)
    random.seed(0)
    data = _feeder(DEV)
    ckpt = str(tmp_path / "checkpoint")
    with open(ckpt + "_args.json", "w") as fh:
        json.dump({"hiddenEncoder": hidden, "hiddenGar": hidden, "arMode": "GRU", "nLevelsGRU": 1, "encoder_type": "cpc",
                   "normMode": "layerNorm", "samplingType": "uniform", "cpc_mode": None}, fh)
    logs = {"epoch": [], "iter": [], "saveStep": 1, "logging_step": 1000}
    before = model.gEncoder.conv0.weight.detach().clone()
    run(data, data, 8, "uniform", model, crit, 2, ckpt, opt, sched, logs)
    assert logs["epoch"] == [0, 1] and len(logs["locLoss_train"]) == 2 and len(logs["locAcc_val"]) == 2
    assert len(logs["locLoss_train"][0]) == 12 and all(np.isfinite(logs["locLoss_val"][1]))
    assert not torch.equal(before, model.gEncoder.conv0.weight.detach())
    shadow = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=2e-4)     # same schedule on a plain optimiser
    shadow_sched = buildScheduler(shadow, schedulerStep=2, schedulerRamp=2)
    for _ in range(2):
        shadow.step()
        shadow_sched.step()
    assert opt.param_groups[0]["lr"] == shadow.param_groups[0]["lr"]
    for epoch in (0, 1):
        sd = torch.load(f"{ckpt}_{epoch}.pt", map_location="cpu")
        assert set(sd) == {"gEncoder", "cpcCriterion", "optimizer", "best"}
    path, saved_logs, _args = getCheckpointData(str(tmp_path))
    assert path.endswith("checkpoint_1.pt") and saved_logs["epoch"] == [0, 1]
    # resume: nothing to do for nEpoch = 2, one more epoch for nEpoch = 3
    run(data, data, 8, "uniform", model, crit, 2, ckpt, opt, sched, saved_logs)
    assert saved_logs["epoch"] == [0, 1]
    run(data, data, 8, "uniform", model, crit, 3, ckpt, opt, sched, saved_logs)
    assert saved_logs["epoch"] == [0, 1, 2] and os.path.exists(f"{ckpt}_2.pt")
    reloaded = loadModel([f"{ckpt}_2.pt"])[0]
    assert torch.equal(reloaded.gEncoder.conv0.weight.cpu(), model.gEncoder.conv0.weight.detach().cpu())


@pytest.mark.parametrize("name", ["tangled", "bidir"])
def test_bidirectional_context_networks_vs_reference_golden(golden, name):
    """BiDIRARTangled (cpc_mode='bert', model.py:219-241) and BiDIRAR (model.py:244-272) on the GRU kernels."""
    from cpc2_amd.model import BiDIRAR, BiDIRARTangled
    g = golden("g15_bidirectional_ar.npz")
    hin, hout, layers, n, t_len = (int(v) for v in g["cfg"])
    net = (BiDIRARTangled if name == "tangled" else BiDIRAR)(hin, hout, layers)
    sd = {k[len(name) + 7:]: t(g[k]) for k in g.files if k.startswith(f"{name}_param.")}
    assert sorted(sd) == sorted(net.state_dict())
    net.load_state_dict(sd)
    net = net.to(DEV)
    assert net.getDimOutput() == hout
    x = synth.features((n, t_len, hin), 131, relu=True).to(DEV).requires_grad_(True)
    out = net(x)
    assert_close(out, t(g[f"{name}_out"]), 1e-5, "out")
    (out * synth.features((n, t_len, hout), 132).to(DEV)).sum().backward()
    assert_close(x.grad, t(g[f"{name}_dx"]), 1e-4, "dx")
    for k, p in net.named_parameters():
        assert_close(p.grad, t(g[f"{name}_grad." + k]), 1e-4, f"grad {k}")


def _full_size_model(hidden, layers, ar):
    """(model on the GPU in eval mode, its parameters as the oracle takes them) for a BASELINE configuration's context network."""
    mp = synth.encoder_params(hidden, 31)
    if ar == "transformer":
        from cpc2_amd.transformers import buildTransformerAR
        for layer in range(layers):
            mp.update(synth.transformer_params(hidden, hidden, 128, 32 + layer, prefix=f"gAR.{layer}."))
        model = cpc2_amd.CPCModel(cpc2_amd.CPCEncoder(hidden), buildTransformerAR(hidden, hidden, layers, 128, False))
        sd = dict(mp)
        sd.update({kk: v for kk, v in model.state_dict().items() if kk.endswith(".z") or kk.endswith(".mask")})
        model.load_state_dict(sd)
    else:
        mp.update(synth.gru_params(hidden, hidden, layers, 32))
        model = cpc2_amd.CPCModel(cpc2_amd.CPCEncoder(hidden), cpc2_amd.CPCAR(hidden, hidden, False, layers))
        model.load_state_dict(mp)
    return model.to(DEV).eval(), mp


@pytest.mark.parametrize("hidden,layers,ar", [(256, 1, "GRU"), (512, 2, "GRU"), (256, 1, "transformer")])
def test_full_size_step_is_window_independent(hidden, layers, ar):
    """BASELINE config C2 / C5 / C4 sizes (128 windows of 20480 samples through encoder + context network): every op up to the
    criterion is per window, so a window's features must not depend on which other windows share the batch.  Not bit for bit: the
    last two convolutions have few enough tiles that their GEMMs split K over workgroups (a split that depends on the batch);
    anything leaking between windows would show at the 1e-1 level, rounding stays below 1e-5."""
    model, _mp = _full_size_model(hidden, layers, ar)
    x = synth.audio_windows(128, 20480, 33).to(DEV)
    with torch.no_grad():
        c_all, z_all, _ = model(x, None)
        c_lo, z_lo, _ = model(x[:64].contiguous(), None)
        c_hi, z_hi, _ = model(x[64:].contiguous(), None)
        c_one, z_one, _ = model(x[77:78].contiguous(), None)
    assert torch.isfinite(c_all).all() and float(z_all.abs().max()) > 0
    assert_close(torch.cat([z_lo, z_hi]), z_all, 1e-5, "z, two halves")
    assert_close(torch.cat([c_lo, c_hi]), c_all, 1e-5, "c, two halves")
    assert_close(z_one, z_all[77:78], 1e-5, "z, one window")
    assert_close(c_one, c_all[77:78], 1e-5, "c, one window")


def test_three_term_gemm_mode_keeps_the_loss_within_the_north_star_tolerance():
    """cpc_gemm_set_mode(2) (opt-in: the encoder's convolution products without the three smallest terms of the split) against
    the exact mode -- which the oracle tests hold to the reference at this width -- over four Adam steps at hidden 256: every loss
    within 1e-3 relative, the bar BASELINE.json states (measured: ~1e-5), and not identical (the mode does change the kernels)."""
    lib = _lib.load()
    hidden, b, k, nn, steps = 256, 6, 12, 32, 4
    curves = {}
    for mode in (0, 2):
        prev = lib.cpc_gemm_set_mode(mode)
        try:
            assert lib.cpc_gemm_set_mode(-1) == mode
            mp = synth.encoder_params(hidden, 21)
            mp.update(synth.gru_params(hidden, hidden, 1, 22))
            model = cpc2_amd.CPCModel(cpc2_amd.CPCEncoder(hidden), cpc2_amd.CPCAR(hidden, hidden, False, 1))
            model.load_state_dict(mp)
            crit = cpc2_amd.CPCUnsupersivedCriterion(k, hidden, hidden, nn, rnnMode="linear", sizeInputSeq=128)
            crit.load_state_dict(synth.predictor_params(k, hidden, hidden, 23))
            model, crit = model.to(DEV), crit.to(DEV)
            opt = buildOptimizer(model, crit, lr=2e-4)
            crit.seed(5)
            x = synth.audio_windows(b, 20480, 24).to(DEV)
            label = torch.zeros(b, dtype=torch.long, device=DEV)
            curve = []
            for _ in range(steps):
                tot, losses, _acc = cpcStep(x, x, label, model, crit)
                tot.backward()
                opt.step()
                opt.zero_grad()
                curve.append(losses.detach())
            curves[mode] = torch.cat(curve).double().cpu()
        finally:
            lib.cpc_gemm_set_mode(prev)
    err = float(((curves[2] - curves[0]).abs() / curves[0].abs()).max())
    assert err <= 1e-3, f"three-term mode: loss curve deviates by {err:.2e} relative"
    assert err > 0.0, "mode 2 ran the exact kernels"
    print(f"three-term mode vs exact mode: max relative loss deviation {err:.2e}")


def test_training_steps_are_reproducible_bit_for_bit():
    """No fp32 atomics are left on the step's path (criterion dz from sorted lists, K splits reduced in a fixed order):
    the same seeds give the same parameters after three steps, bit for bit -- at a small size where the K splits and the
    streaming recurrent kernels are used, and at a size that takes the cooperative GRU."""
    for hidden, b, t_windows in ((64, 3, 20480), (256, 8, 20480)):
        finals = []
        for _run in range(2):
            mp = synth.encoder_params(hidden, 21)
            mp.update(synth.gru_params(hidden, hidden, 1, 22))
            model = cpc2_amd.CPCModel(cpc2_amd.CPCEncoder(hidden), cpc2_amd.CPCAR(hidden, hidden, False, 1))
            model.load_state_dict(mp)
            crit = cpc2_amd.CPCUnsupersivedCriterion(12, hidden, hidden, 16, rnnMode="linear", sizeInputSeq=128)
            crit.load_state_dict(synth.predictor_params(12, hidden, hidden, 23))
            model, crit = model.to(DEV), crit.to(DEV)
            opt = buildOptimizer(model, crit, lr=2e-4)
            crit.seed(5)
            x = synth.audio_windows(b, t_windows, 24).to(DEV)
            label = torch.zeros(b, dtype=torch.long, device=DEV)
            for _ in range(3):
                tot, _losses, _acc = cpcStep(x, x, label, model, crit)
                tot.backward()
                opt.step()
                opt.zero_grad()
            finals.append(opt.flat.detach().clone())
        assert torch.equal(finals[0], finals[1]), f"hidden {hidden}: parameters differ between two identical runs"


@pytest.mark.parametrize("form", ["context", "strict", "dedup"])
def test_deferred_criterion_backward_gives_the_same_step_bit_for_bit(monkeypatch, form):
    """cpc_infonce_backward with deferred = 1 + cpc_infonce_join (dz and the predictor weight gradients on the library's side stream,
    beside the recurrent backward; joined where autograd sums the encoder output's gradient) runs the SAME kernels as the
    immediate form: every gradient and the parameters after two steps are equal bit for bit -- with cpcStep's default (context
    network on the b context windows: the criterion differentiates with respect to the target half of split_windows), with the
    reference's own 2b-window dataflow (strict: with respect to the full encoder output, rows b.. only) and with dedup."""
    from cpc2_amd import _route as route_mod, criterion as crit_mod
    hidden, b = 256, 6
    dedup, strict = form == "dedup", form == "strict"
    results = []
    for defer in (True, False):
        if defer:
            monkeypatch.delenv("CPC_NCE_NO_DEFER", raising=False)
        else:
            monkeypatch.setenv("CPC_NCE_NO_DEFER", "1")
        mp = synth.encoder_params(hidden, 21)
        mp.update(synth.gru_params(hidden, hidden, 1, 22))
        model = cpc2_amd.CPCModel(cpc2_amd.CPCEncoder(hidden), cpc2_amd.CPCAR(hidden, hidden, False, 1))
        model.load_state_dict(mp)
        crit = cpc2_amd.CPCUnsupersivedCriterion(12, hidden, hidden, 32, rnnMode="linear", sizeInputSeq=128)
        crit.load_state_dict(synth.predictor_params(12, hidden, hidden, 23))
        model, crit = model.to(DEV), crit.to(DEV)
        opt = buildOptimizer(model, crit, lr=2e-4)
        crit.seed(5)
        x = synth.audio_windows(b, 20480, 24).to(DEV)
        label = torch.zeros(b, dtype=torch.long, device=DEV)
        seen = []
        real = crit_mod._InfoNCEFn.apply

        def spy(*a):
            seen.append(a[5])
            return real(*a)
        monkeypatch.setattr(crit_mod._InfoNCEFn, "apply", staticmethod(spy))
        grads = []
        for _ in range(2):
            tot, _losses, _acc = cpcStep(x, x, label, model, crit, dedup=dedup, strict=strict)
            tot.backward()
            assert not route_mod._deferred, "a deferred backward is still pending after the backward pass"
            grads.append(opt.flat_grad.detach().clone())
            opt.step()
            opt.zero_grad()
        monkeypatch.setattr(crit_mod._InfoNCEFn, "apply", real)
        assert all((d is not None) == defer for d in seen), seen
        if defer:
            assert seen[0] == ((b, b) if strict else (0, b))
        results.append((grads, opt.flat.detach().clone()))
    for step in range(2):
        assert torch.equal(results[0][0][step], results[1][0][step]), f"step {step}: gradients differ between the two forms"
    assert torch.equal(results[0][1], results[1][1])


def _step_model(hidden, layers, mode, nneg, seed=3):
    torch.manual_seed(seed)
    if mode == "transformer":
        from cpc2_amd.transformers import buildTransformerAR
        ar = buildTransformerAR(hidden, hidden, layers, 128, False)
    else:
        ar = cpc2_amd.CPCAR(hidden, hidden, False, layers, mode=mode)
    model = cpc2_amd.CPCModel(cpc2_amd.CPCEncoder(hidden), ar).to(DEV)
    crit = cpc2_amd.CPCUnsupersivedCriterion(12, hidden, hidden, nneg, rnnMode="linear", sizeInputSeq=128).to(DEV)
    return model, crit


@pytest.mark.parametrize("name,hidden,layers,mode,b,nneg", [("gru", 256, 1, "GRU", 6, 32), ("gru_x2_512", 512, 2, "GRU", 5, 64),
                                                          ("lstm", 256, 1, "LSTM", 6, 32), ("transformer", 256, 1, "transformer", 4, 32),
                                                          ("transformer_x2", 256, 2, "transformer", 3, 32), ("gru_64", 64, 1, "GRU", 3, 16),
                                                          ("rnn", 256, 1, "RNN", 4, 32), ("gru_many", 256, 1, "GRU", 40, 32)])
def test_context_network_on_the_context_windows_only_is_the_reference_step(name, hidden, layers, mode, b, nneg):
    """train.py:99-103 keeps c_feature[:b] and encoded_data[b:] of the model's 2b-window outputs, criterion.py:296 the first
    W = T - nPredicts frames of that context.  cpcStep's default form runs the context network on the b context windows only and,
    when it is recurrent, over those W frames only; `strict=True` is the reference's own dataflow (CPCModel.forward on all 2b
    windows, T frames).  With past != future, three Adam steps (transformer: dropout 0.1 on, the masks are keyed by element position):
    losses, every gradient and the parameters agree -- bit for bit where the row count does not change a K split or a
    summation order, else to rounding (2e-6 of scale; parameters within 2 % of the distance Adam moved them)."""
    lr, steps = 2e-4, 3
    res = {}
    for form in ("context", "strict"):
        model, crit = _step_model(hidden, layers, mode, nneg)
        opt = buildOptimizer(model, crit, lr=lr)
        crit.seed(5)
        torch.manual_seed(11)                                   # (the transformer's dropout stream)
        past = synth.audio_windows(b, 20480, 24).to(DEV)
        future = synth.audio_windows(b, 20480, 25).to(DEV)
        label = torch.zeros(b, dtype=torch.long, device=DEV)
        init = opt.flat.detach().clone()
        losses, grads = [], []
        for _ in range(steps):
            tot, ls, _acc = cpcStep(past, future, label, model, crit, strict=form == "strict")
            tot.backward()
            losses.append(ls.detach().clone())
            grads.append(opt.flat_grad.detach().clone())
            opt.step()
            opt.zero_grad()
        _lib.check(_lib.load().cpc_async_error_check(_lib.stream_ptr(torch.device(DEV))), "async error check")
        res[form] = (torch.cat(losses), grads, opt.flat.detach().clone(), init, opt)
    got, ref = res["context"], res["strict"]
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[2]).all()
    exact = torch.equal(got[0], ref[0]) and all(torch.equal(a, c) for a, c in zip(got[1], ref[1])) and torch.equal(got[2], ref[2])
    print(f"{name}: context-windows-only vs strict 2b form: {'bit-identical' if exact else 'equal to rounding'}")
    assert_close(got[0][:12], ref[0][:12], 2e-6, "losses, step 0")
    assert_close(got[0], ref[0], 2e-5, "losses")
    opt = got[4]
    for step in range(steps):
        for prm, off in zip(opt.params, opt.offsets):            # per parameter tensor: each against its own scale
            n = prm.numel()
            # (after an Adam step the two runs' parameters differ by rounding-sized gradients' worth, and a ReLU decision that flips
            #  with them moves a gradient by ~1e-3 of its scale: section 2 of DESIGN.md; step 0 is the sharp comparison)
            assert_close(got[1][step][off:off + n], ref[1][step][off:off + n], 4e-6 if step == 0 else 5e-2,
                         f"step {step}: gradient at flat offset {off} ({tuple(prm.shape)})")
    moved = (ref[2] - ref[3]).abs()
    assert float(moved.max()) > 0.5 * lr * steps
    diff = (got[2] - ref[2]).abs()
    # (Adam moves an element by ~lr per step whatever its gradient's size: one whose gradient is rounding noise may go the other way)
    assert float(diff.max()) <= 1.0 * lr * steps, f"a parameter ended {float(diff.max()):.2e} away"
    assert float(diff.mean()) <= 0.02 * float(moved.mean()), f"mean parameter distance {float(diff.mean()):.2e} vs moved {float(moved.mean()):.2e}"


@pytest.mark.parametrize("config", ["small", "transformer"])
def test_context_windows_only_form_matches_strict_along_a_trajectory_at_full_batch(config):
    """The bench workload itself (b = 64 windows, CPC-small / transformer AR in training mode): along ONE training trajectory of
    cpcStep's default form, every 20 steps the gradient of the reference's 2b-window dataflow (strict=True) is evaluated on the SAME
    parameters, negative indices and dropout seed: losses equal to 1e-6, every parameter gradient to 2e-5 of its tensor's scale
    (measured 4e-7 .. 7e-6).  Two runs of the two forms drift apart over hundreds of Adam steps on this pure-noise input (rounding-sized
    gradient differences grow like any perturbation of that trajectory: profiles/r05_soak.txt) -- this is the check that the drift is
    not a difference between the forms."""
    import bench
    cfg = bench.CONFIGS[config]
    dev = torch.device(DEV)
    mA, cA, oA = bench.build(cfg, dev)
    mB, cB, oB = bench.build(cfg, dev)
    x = (0.05 * torch.randn(64, 1, bench.WINDOW, generator=torch.Generator().manual_seed(1000))).to(dev)
    label = torch.zeros(64, dtype=torch.long, device=dev)
    names = [n for n, _ in list(cA.named_parameters()) + list(mA.named_parameters())]
    checked = 0
    for step in range(41):
        cA.seed(5000 + step)
        torch.manual_seed(step)                  # (a transformer layer draws its dropout seed from torch's CPU generator)
        tot, lA, _ = cpcStep(x, x, label, mA, cA)
        tot.backward()
        if step % 20 == 0:
            oB.flat.copy_(oA.flat)
            cB.seed(5000 + step)
            torch.manual_seed(step)
            totB, lB, _ = cpcStep(x, x, label, mB, cB, strict=True)
            totB.backward()
            assert_close(lA, lB, 1e-6, f"step {step}: losses")
            for name, p, off in zip(names, oA.params, oA.offsets):
                n = p.numel()
                assert_close(oA.flat_grad[off:off + n], oB.flat_grad[off:off + n], 2e-5, f"step {step}: grad {name}")
            oB.zero_grad()
            checked += 1
        oA.step()
        oA.zero_grad()
    assert checked == 3 and float(lA.mean()) < 4.8598
    _lib.check(_lib.load().cpc_async_error_check(_lib.stream_ptr(dev)), "async error check")


def test_context_windows_only_form_is_refused_where_it_would_change_the_observable():
    """The reduced dataflow is cpcStep's own and only for the bare CPCModel without state across calls: span masking (numpy draws
    over all 2b rows), keepHidden (the stored state covers 2b windows) and any wrapper keep the reference's 2b-window call."""
    from cpc2_amd.train import _context_frames_only, _context_windows_only
    from cpc2_amd.transformers import buildTransformerAR
    hidden = 64
    enc = cpc2_amd.CPCEncoder(hidden)
    # the time axis (criterion.py:296 keeps cFeature[:, :windowSize]): only a causal recurrent network without carried state stops
    # after the W frames the criterion reads; a reversed one, the transformer (its blocks are padded to sizeSeq anyway), a criterion
    # in reverse mode or a wrapped one keep all T frames
    crit12 = cpc2_amd.CPCUnsupersivedCriterion(12, hidden, hidden, 16, rnnMode="linear", sizeInputSeq=128)
    assert _context_frames_only(cpc2_amd.CPCModel(enc, cpc2_amd.CPCAR(hidden, hidden, False, 1)), crit12, 128) == 116
    assert _context_frames_only(cpc2_amd.CPCModel(enc, cpc2_amd.CPCAR(hidden, hidden, False, 2, mode="LSTM")), crit12, 128) == 116
    assert _context_frames_only(cpc2_amd.CPCModel(enc, cpc2_amd.CPCAR(hidden, hidden, False, 1, reverse=True)), crit12, 128) == 0
    assert _context_frames_only(cpc2_amd.CPCModel(enc, cpc2_amd.CPCAR(hidden, hidden, True, 1)), crit12, 128) == 0
    assert _context_frames_only(cpc2_amd.CPCModel(enc, buildTransformerAR(hidden, hidden, 1, 128, False)), crit12, 128) == 0
    rev = cpc2_amd.CPCUnsupersivedCriterion(12, hidden, hidden, 16, mode="reverse", rnnMode="linear", sizeInputSeq=128)
    assert _context_frames_only(cpc2_amd.CPCModel(enc, cpc2_amd.CPCAR(hidden, hidden, False, 1)), rev, 128) == 0
    assert _context_frames_only(cpc2_amd.CPCModel(enc, cpc2_amd.CPCAR(hidden, hidden, False, 1)), torch.nn.DataParallel(crit12), 128) == 0
    assert _context_windows_only(cpc2_amd.CPCModel(enc, cpc2_amd.CPCAR(hidden, hidden, False, 1)))
    assert _context_windows_only(cpc2_amd.CPCModel(enc, cpc2_amd.CPCAR(hidden, hidden, False, 2, mode="LSTM")))
    assert not _context_windows_only(cpc2_amd.CPCModel(enc, cpc2_amd.CPCAR(hidden, hidden, True, 1)))
    assert not _context_windows_only(cpc2_amd.CPCModel(enc, cpc2_amd.CPCAR(hidden, hidden, False, 1), mask_prob=0.05))
    assert not _context_windows_only(torch.nn.DataParallel(cpc2_amd.CPCModel(enc, cpc2_amd.CPCAR(hidden, hidden, False, 1))))
    # and with keepHidden the two forms are used as the reference would: the state of all 2b windows is carried
    model = cpc2_amd.CPCModel(enc, cpc2_amd.CPCAR(hidden, hidden, True, 1)).to(DEV)
    crit = cpc2_amd.CPCUnsupersivedCriterion(12, hidden, hidden, 16, rnnMode="linear", sizeInputSeq=128).to(DEV)
    x = synth.audio_windows(2, 20480, 24).to(DEV)
    with torch.no_grad():
        cpcStep(x, x, torch.zeros(2, dtype=torch.long, device=DEV), model, crit)
    assert model.gAR.hidden.shape == (1, 4, hidden)


_DEFER_LAYERS_SCRIPT = """
import sys, torch
sys.path.insert(0, {root!r})
import cpc2_amd
from cpc2_amd import _lib
from cpc2_amd import _route as route_mod
from cpc2_amd.train import buildOptimizer, cpcStep
from oracle import synth
hidden, b, mode = 512, 32, {mode!r}
torch.manual_seed(3)
model = cpc2_amd.CPCModel(cpc2_amd.CPCEncoder(hidden), cpc2_amd.CPCAR(hidden, hidden, False, 2, mode=mode)).to("cuda:0")
crit = cpc2_amd.CPCUnsupersivedCriterion(12, hidden, hidden, 256, rnnMode="linear", sizeInputSeq=128).to("cuda:0")
opt = buildOptimizer(model, crit, lr=2e-4)
crit.seed(5)
x = synth.audio_windows(b, 20480, 24).to("cuda:0")
label = torch.zeros(b, dtype=torch.long, device="cuda:0")
for _ in range(2):
    tot, _l, _a = cpcStep(x, x, label, model, crit)
    tot.backward()
    assert not route_mod._deferred
    opt.step()
    opt.zero_grad()
_lib.check(_lib.load().cpc_async_error_check(_lib.stream_ptr(torch.device("cuda:0"))), "async error check")
torch.save(opt.flat.detach().cpu(), {dst!r})
"""


@pytest.mark.parametrize("mode", ["GRU", "LSTM"])
def test_deferred_backward_with_two_recurrent_layers_at_many_windows(tmp_path, mode):
    """Round-3 advisor finding: with two recurrent layers (CPC-large: hidden 512) the deferred dz sum and predictor weight gradient
    start on the side stream behind layer 1's cooperative backward kernel and can still hold CUs when layer 0's -- which needs
    every workgroup resident -- is launched.  64 windows through the context network (b = 32, reference semantics), GRU and LSTM:
    two deferred training steps end with a clean asynchronous error word and the same parameters, bit for bit, as the immediate
    form (CPC_NCE_NO_DEFER=1, its own process)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for form, env in (("deferred", {}), ("immediate", {"CPC_NCE_NO_DEFER": "1"})):
        dst = str(tmp_path / f"{form}.pt")
        e = dict(os.environ, PYTHONPATH=root, **env)
        if form == "deferred":
            e.pop("CPC_NCE_NO_DEFER", None)
        r = subprocess.run([sys.executable, "-c", _DEFER_LAYERS_SCRIPT.format(root=root, mode=mode, dst=dst)], env=e, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[form] = torch.load(dst)
    assert torch.isfinite(res["deferred"]).all()
    assert torch.equal(res["deferred"], res["immediate"]), f"{mode} x2: parameters differ between the deferred and the immediate backward"


def _spied_criterion_calls(monkeypatch, run):
    """Runs `run()` with _InfoNCEFn.apply spied: the `defer` argument of every call."""
    from cpc2_amd import criterion as crit_mod
    seen = []
    real = crit_mod._InfoNCEFn.apply

    def spy(*a):
        seen.append(a[5])
        return real(*a)
    monkeypatch.setattr(crit_mod._InfoNCEFn, "apply", staticmethod(spy))
    try:
        out = run()
    finally:
        monkeypatch.setattr(crit_mod._InfoNCEFn, "apply", real)
    return seen, out


def test_criterion_backward_is_deferred_only_inside_the_callers_scope(monkeypatch):
    """Round-3 advisor finding: the deferral must be the caller's explicit promise (cpcStep's `deferred_backward` scope), not
    something a tensor attribute switches on.  (1) model and criterion called directly, the way the reference's train.py
    does, with a SECOND loss term on the encoder output -- autograd sums the two gradients of that tensor as soon as both
    exist, i.e. before a join: nothing may be deferred, and the gradient is the sum of the two terms' own gradients.
    (2) inside cpcStep, a predictor weight with a tensor hook (what DDP's reducer amounts to): not deferred either."""
    from cpc2_amd import _route as route_mod
    hidden, b = 256, 4
    mp = synth.encoder_params(hidden, 21)
    mp.update(synth.gru_params(hidden, hidden, 1, 22))
    model = cpc2_amd.CPCModel(cpc2_amd.CPCEncoder(hidden), cpc2_amd.CPCAR(hidden, hidden, False, 1))
    model.load_state_dict(mp)
    crit = cpc2_amd.CPCUnsupersivedCriterion(12, hidden, hidden, 32, rnnMode="linear", sizeInputSeq=128)
    crit.load_state_dict(synth.predictor_params(12, hidden, hidden, 23))
    model, crit = model.to(DEV), crit.to(DEV)
    opt = buildOptimizer(model, crit, lr=2e-4)
    x = synth.audio_windows(b, 20480, 24).to(DEV)
    label = torch.zeros(b, dtype=torch.long, device=DEV)
    probe = torch.randn(b, 128, hidden, generator=torch.Generator().manual_seed(9)).to(DEV)

    def direct(with_nce, with_extra):
        crit.seed(5)
        opt.zero_grad()
        c, z, _ = model(x, label)
        assert getattr(route_mod.mark(z), "join", False)         # the mark is there -- and must not be what decides
        tot = 0.0
        if with_nce:
            losses, _acc = crit(c, z, label)
            tot = tot + losses.sum()
        if with_extra:
            tot = tot + (z * probe).sum() * 1e-3
        tot.backward()
        assert not route_mod._deferred
        opt._gather_stray_grads()
        return opt.flat_grad.detach().clone()
    seen, both = _spied_criterion_calls(monkeypatch, lambda: direct(True, True))
    assert seen == [None], seen
    only_nce, only_extra = direct(True, False), direct(False, True)
    ref = only_nce.double() + only_extra.double()
    assert float((both.double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    assert float(only_extra.abs().max()) > 0

    # (2) cpcStep opens the scope; a hook on a predictor weight closes it again
    def step():
        crit.seed(5)
        opt.zero_grad()
        tot, _l, _a = cpcStep(x[:2], x[:2], label[:2], model, crit)
        tot.backward()
        opt._gather_stray_grads()
        return opt.flat_grad.detach().clone()
    seen, g_deferred = _spied_criterion_calls(monkeypatch, step)
    assert seen == [(0, 2)], seen            # (the target half of split_windows: windows 0.. of the tensor the criterion is given)
    touched = []
    handle = crit.wPrediction.predictors[3].weight.register_hook(lambda g: touched.append(float(g.abs().sum())))
    seen, g_hooked = _spied_criterion_calls(monkeypatch, step)
    handle.remove()
    assert seen == [None] and len(touched) == 1 and touched[0] > 0, (seen, touched)
    assert torch.equal(g_deferred, g_hooked)


def test_recurrent_weight_gradients_are_deferred_only_inside_the_callers_scope(monkeypatch):
    """cpc_gru_backward / cpc_lstm_backward / cpc_encoder_backward with deferred = 1 (parameter-gradient work on the library's side
    stream; counted below: the calls whose `deferred` argument, the one in front of the stream, is non-zero):
    (1) cpcStep on the bare model defers them, and every gradient of the step is bit-identical to the immediate form's;
    (2) model called directly (the reference's train.py), or a tensor hook on one of those weights: not deferred;
    (3) two GRU layers: layer 1's gradients on the caller's stream, layer 0's deferred -- same bits again."""
    from cpc2_amd import model as model_mod
    for layers, hidden, b, mode in ((1, 256, 2, "GRU"), (2, 256, 2, "GRU"), (1, 256, 2, "LSTM")):
        mp = synth.encoder_params(hidden, 41)
        mp.update((synth.gru_params if mode == "GRU" else synth.lstm_params)(hidden, hidden, layers, 42))
        model = cpc2_amd.CPCModel(cpc2_amd.CPCEncoder(hidden), cpc2_amd.CPCAR(hidden, hidden, False, layers, mode=mode))
        model.load_state_dict(mp)
        crit = cpc2_amd.CPCUnsupersivedCriterion(12, hidden, hidden, 32, rnnMode="linear", sizeInputSeq=128)
        crit.load_state_dict(synth.predictor_params(12, hidden, hidden, 43))
        model, crit = model.to(DEV), crit.to(DEV)
        opt = buildOptimizer(model, crit, lr=2e-4)
        x = synth.audio_windows(b, 20480, 44).to(DEV)
        label = torch.zeros(b, dtype=torch.long, device=DEV)
        lib = _lib.load()
        calls, enc_calls = [], []
        rec_name = "cpc_gru_backward" if mode == "GRU" else "cpc_lstm_backward"
        real, real_enc = getattr(lib, rec_name), lib.cpc_encoder_backward

        def spy(*a):
            if a[-2]:
                calls.append(1)
            return real(*a)

        def spy_enc(*a):
            if a[-2]:
                enc_calls.append(1)
            return real_enc(*a)
        monkeypatch.setattr(lib, rec_name, spy)
        monkeypatch.setattr(lib, "cpc_encoder_backward", spy_enc)

        def grads(how):
            crit.seed(5)
            opt.zero_grad()
            del calls[:]
            del enc_calls[:]
            if how == "step":                              # (strict: the same 2b-window dataflow as the direct calls below)
                tot, _l, _a = cpcStep(x, x, label, model, crit, strict=True)
            elif how == "direct":                          # the reference's own sequence of calls: no scope
                c, z, _ = model(torch.cat([x, x]), label)
                losses, _a = crit(c[:b], z[b:], label)
                tot = losses.sum()
            tot.backward()
            assert not model_mod._tail                     # joined by the end of the backward pass
            opt._gather_stray_grads()
            torch.cuda.synchronize()
            return opt.flat_grad.detach().clone(), (len(calls), len(enc_calls))
        g_step, n_step = grads("step")
        g_direct, n_direct = grads("direct")
        assert n_step == (1, 1) and n_direct == (0, 0), (n_step, n_direct)      # (recurrent backward, encoder backward)
        assert torch.equal(g_step, g_direct) and float(g_step.abs().max()) > 0
        touched = []
        handle = model.gAR.baseNet.weight_hh_l0.register_hook(lambda g: touched.append(float(g.abs().sum())))
        g_hooked, n_hooked = grads("step")
        handle.remove()
        assert n_hooked == (0, 1) and len(touched) == 1 and touched[0] > 0
        assert torch.equal(g_step, g_hooked)
        handle = model.gEncoder.conv2.weight.register_hook(lambda g: touched.append(float(g.abs().sum())))
        g_hooked2, n_hooked2 = grads("step")
        handle.remove()
        assert n_hooked2 == (1, 0) and len(touched) == 2 and touched[1] > 0
        assert torch.equal(g_step, g_hooked2)
        monkeypatch.setattr(lib, rec_name, real)
        monkeypatch.setattr(lib, "cpc_encoder_backward", real_enc)


@pytest.mark.parametrize("n_layers", [1, 2, 3])
def test_transformer_parameter_gradients_are_deferred_inside_the_callers_scope(monkeypatch, n_layers):
    """cpc_transformer_backward with deferred = 1 (arMode='transformer': the layer's seven weight-gradient products, bias sums and column sums
    on the library's side stream): cpcStep on the bare model defers, the model called directly does not, every gradient of the step
    is the same bit for bit -- in training mode (dropout on, same seed) and with the criterion's own deferred backward beside it.
    nLevelsGRU >= 2 (round-4 advisor finding): every TransformerLayer of the nn.Sequential defers on its own, the side stream
    still reads layer l's buffers while layer l - 1 runs its backward: each pending call has a scratch buffer of its own."""
    from cpc2_amd import model as model_mod
    from cpc2_amd.transformers import buildTransformerAR
    hidden, b = 256, 2
    mp = synth.encoder_params(hidden, 51)
    for layer in range(n_layers):
        mp.update(synth.transformer_params(hidden, hidden, 128, 52 + 10 * layer, prefix=f"gAR.{layer}."))
    model = cpc2_amd.CPCModel(cpc2_amd.CPCEncoder(hidden), buildTransformerAR(hidden, hidden, n_layers, 128, False))
    sd = dict(mp)
    sd.update({kk: v for kk, v in model.state_dict().items() if kk.endswith(".z") or kk.endswith(".mask")})
    model.load_state_dict(sd)
    crit = cpc2_amd.CPCUnsupersivedCriterion(12, hidden, hidden, 32, rnnMode="linear", sizeInputSeq=128)
    crit.load_state_dict(synth.predictor_params(12, hidden, hidden, 53))
    model, crit = model.to(DEV).train(), crit.to(DEV).train()
    opt = buildOptimizer(model, crit, lr=2e-4)
    x = synth.audio_windows(b, 20480, 54).to(DEV)
    label = torch.zeros(b, dtype=torch.long, device=DEV)
    lib = _lib.load()
    calls = []
    real = lib.cpc_transformer_backward

    def spy(*a):
        if a[-2]:                                          # (`deferred`, the argument in front of the stream)
            calls.append(1)
        return real(*a)
    monkeypatch.setattr(lib, "cpc_transformer_backward", spy)

    def grads(how):
        crit.seed(5)
        torch.manual_seed(11)                              # (the layer draws its dropout seed from torch's generator)
        opt.zero_grad()
        del calls[:]
        if how == "step":
            tot, _l, _a = cpcStep(x, x, label, model, crit, strict=True)      # (the same 2b-window dataflow as the direct call)
        else:
            c, z, _ = model(torch.cat([x, x]), label)
            losses, _a = crit(c[:b], z[b:], label)
            tot = losses.sum()
        tot.backward()
        assert not model_mod._tail
        opt._gather_stray_grads()
        torch.cuda.synchronize()
        return opt.flat_grad.detach().clone(), len(calls)
    for _rep in range(2):                                  # (twice: the second pass finds every buffer in place)
        g_step, n_step = grads("step")
        g_direct, n_direct = grads("direct")
        assert (n_step, n_direct) == (n_layers, 0)
        assert torch.equal(g_step, g_direct) and float(g_step.abs().max()) > 0
    monkeypatch.setattr(lib, "cpc_transformer_backward", real)


def test_seeded_backward_of_the_summed_losses_is_the_plain_one():
    """cpc2_amd.train.backward(totLoss) (train.py:106,109 without the one-element kernels autograd puts between the criterion's
    forward and backward: a cached 1.0 as the root gradient, a cached vector of ones out of the sum's backward) gives every
    gradient of `allLosses.sum().backward()` bit for bit -- and a caller who scales the loss still gets the scaled gradient."""
    from cpc2_amd.train import backward as seeded_backward, sum_losses
    hidden, b = 256, 2
    mp = synth.encoder_params(hidden, 31)
    mp.update(synth.gru_params(hidden, hidden, 1, 32))
    model = cpc2_amd.CPCModel(cpc2_amd.CPCEncoder(hidden), cpc2_amd.CPCAR(hidden, hidden, False, 1))
    model.load_state_dict(mp)
    crit = cpc2_amd.CPCUnsupersivedCriterion(12, hidden, hidden, 32, rnnMode="linear", sizeInputSeq=128)
    crit.load_state_dict(synth.predictor_params(12, hidden, hidden, 33))
    model, crit = model.to(DEV), crit.to(DEV)
    opt = buildOptimizer(model, crit, lr=2e-4)
    x = synth.audio_windows(b, 20480, 34).to(DEV)
    label = torch.zeros(b, dtype=torch.long, device=DEV)

    def grads(how):
        crit.seed(5)
        opt.zero_grad()
        tot, losses, _a = cpcStep(x, x, label, model, crit)
        if how == "plain":
            losses.sum().backward()
        elif how == "seeded":
            assert tot.grad_fn is not None and type(tot.grad_fn).__name__.startswith("_SumLosses")
            seeded_backward(tot)
        else:
            (3.0 * sum_losses(losses)).backward()
        opt._gather_stray_grads()
        return opt.flat_grad.detach().clone(), float(tot)
    g_plain, t_plain = grads("plain")
    g_seeded, t_seeded = grads("seeded")
    g_scaled, _t = grads("scaled")
    assert t_plain == t_seeded and torch.equal(g_plain, g_seeded)
    assert float(g_plain.abs().max()) > 0
    # (a factor of 3 in front of every product moves f32 roundings: 1e-5 of the largest gradient measured, the usual step-level bar)
    assert float((g_scaled.double() - 3.0 * g_plain.double()).abs().max()) <= 5e-5 * float(g_plain.abs().max()) * 3.0


def test_criterion_index_range_is_checked_on_the_device():
    """SURVEY section 5 (criterion.py:264-268's gather): a negative-sample index outside [0, b * t) must not become an out-of-bounds
    gather.  The forward pass replaces it by row 0 and the asynchronous error check reports it; with the same index set to 0 by
    the caller the losses are the same bit for bit, and a clean call leaves the error word alone."""
    lib = _lib.load()
    b, t, k, h, nn = 2, 128, 12, 256, 32
    g = torch.Generator().manual_seed(3)
    c = torch.randn(b, t, h, generator=g).to(DEV)
    z = torch.randn(b, t, h, generator=g).to(DEV)
    wpred = (0.05 * torch.randn(k, h, h, generator=g)).to(DEV)
    ext = torch.randint(0, b * t, (b * (t - k) * nn,), generator=g, dtype=torch.int32)
    st = _lib.stream_ptr(c.device)
    nsaved = lib.cpc_infonce_saved_bytes(b, t, k, h, h, nn)
    nscr = lib.cpc_infonce_scratch_bytes(b, t, k, h, h, nn)

    def forward(idx):
        saved = torch.empty(nsaved, dtype=torch.uint8, device=DEV)
        scr = torch.empty(nscr, dtype=torch.uint8, device=DEV)
        losses, acc = torch.empty(k, device=DEV), torch.empty(k, device=DEV)
        idx = idx.to(DEV)
        _lib.check(lib.cpc_infonce_forward(_lib.ptr(c), _lib.ptr(z), _lib.ptr(wpred), _lib.ptr(idx), None, _lib.ptr(losses), _lib.ptr(acc),
                                           _lib.ptr(saved), _lib.ptr(scr), b, t, t, k, h, h, nn, st), "fwd")
        return losses.cpu(), lib.cpc_async_error_check(st)
    clean, rc = forward(ext)
    assert rc == 0
    bad = ext.clone()
    bad[1234], bad[77] = b * t + 5, -3
    got, rc = forward(bad)
    assert rc != 0 and "indices outside" in lib.cpc_last_error().decode()
    fixed = ext.clone()
    fixed[1234], fixed[77] = 0, 0
    want, rc = forward(fixed)
    assert rc == 0 and torch.equal(got, want) and torch.isfinite(got).all()
    assert not torch.equal(clean, want)


def test_infonce_backward_deferred_c_entry_matches_the_immediate_one():
    """The C entry point itself: cpc_infonce_backward with deferred = 1 + join on the calling stream == deferred = 0, bit for bit; a
    second join is a no-op."""
    from cpc2_amd import _lib
    lib = _lib.load()
    b, t, k, h, nn = 4, 128, 12, 256, 32
    g = torch.Generator().manual_seed(3)
    c = torch.randn(b, t, h, generator=g).to(DEV)
    z = torch.randn(b, t, h, generator=g).to(DEV)
    wpred = (0.05 * torch.randn(k, h, h, generator=g)).to(DEV)
    ext = torch.randint(0, b * t, (b * (t - k) * nn,), generator=g, dtype=torch.int32).to(DEV)
    dl = torch.rand(k, generator=g).to(DEV)
    st = _lib.stream_ptr(c.device)
    nsaved = lib.cpc_infonce_saved_bytes(b, t, k, h, h, nn)
    nscr = lib.cpc_infonce_scratch_bytes(b, t, k, h, h, nn)
    outs = []
    for deferred in (0, 1):
        saved = torch.empty(nsaved, dtype=torch.uint8, device=DEV)
        scr = torch.empty(nscr, dtype=torch.uint8, device=DEV)
        losses, acc = torch.empty(k, device=DEV), torch.empty(k, device=DEV)
        _lib.check(lib.cpc_infonce_forward(_lib.ptr(c), _lib.ptr(z), _lib.ptr(wpred), _lib.ptr(ext), None, _lib.ptr(losses), _lib.ptr(acc),
                                           _lib.ptr(saved), _lib.ptr(scr), b, t, t, k, h, h, nn, st), "fwd")
        dc, dz, dw = torch.empty_like(c), torch.empty_like(z), torch.empty_like(wpred)
        _lib.check(lib.cpc_infonce_backward(_lib.ptr(c), _lib.ptr(z), _lib.ptr(wpred), _lib.ptr(ext), None, _lib.ptr(dl), _lib.ptr(saved),
                                            _lib.ptr(scr), _lib.ptr(dc), _lib.ptr(dz), _lib.ptr(dw), b, t, t, k, h, h, nn, deferred, st), "bwd")
        if deferred:
            _lib.check(lib.cpc_infonce_join(st), "join")
            _lib.check(lib.cpc_infonce_join(st), "join again")
        torch.cuda.synchronize()
        outs.append((dc, dz, dw))
    for name, a, bb in zip(("dc", "dz", "dwpred"), outs[0], outs[1]):
        assert torch.equal(a, bb), name
    assert float(outs[0][1].abs().max()) > 0


def test_unified_entry_points_refuse_inconsistent_arguments():
    """The arguments that replaced the sibling entry points are checked before anything is launched: each call below returns
    CPC_ERR_INVALID (ValueError) with a message of its own and leaves its poisoned outputs untouched."""
    lib = _lib.load()
    st = _lib.stream_ptr(torch.device(DEV))
    nan = float("nan")
    # encoder: hidden 32, two windows of 400 samples
    hidden, n, length = 32, 2, 400
    params = [v.to(DEV).contiguous() for v in synth.encoder_params(hidden, seed=5).values()]
    x = synth.audio_windows(n, length, seed=6).to(DEV)
    z = torch.full((n, lib.cpc_encoder_frames(length), hidden), nan, device=DEV)
    nsaved, nscr = lib.cpc_encoder_saved_bytes(n, length, hidden), lib.cpc_encoder_scratch_bytes(n, length, hidden)
    assert nsaved > 0 and nscr > 0
    saved, scr = torch.empty(nsaved, dtype=torch.uint8, device=DEV), torch.empty(nscr, dtype=torch.uint8, device=DEV)

    def encoder(x_rest, n_first):
        _lib.check(lib.cpc_encoder_forward(_lib.ptr(x), _lib.ptr(x_rest), n_first, _lib.ptr_array(params), _lib.ptr(z), _lib.ptr(saved),
                                           _lib.ptr(scr), n, length, hidden, 1e-5, st), "encoder_forward")
    with pytest.raises(ValueError, match="one input batch"):
        encoder(None, 1)                                   # x_rest = NULL and n_first != n_windows
    with pytest.raises(ValueError, match="first batch"):
        encoder(x[1:], 0)                                  # x_rest set, no window in the first batch
    with pytest.raises(ValueError, match="first batch"):
        encoder(x[1:], n)                                  # x_rest set, every window in the first batch
    # criterion: a context of t - 1 frames is neither the sequence nor the W frames the criterion uses
    b, t, k, nn, dim = 2, 20, 4, 8, 32
    g = torch.Generator().manual_seed(3)
    c, zc = torch.randn(b, t, dim, generator=g).to(DEV), torch.randn(b, t, dim, generator=g).to(DEV)
    wpred = (0.05 * torch.randn(k, dim, dim, generator=g)).to(DEV)
    ext = torch.randint(0, b * t, (b * (t - k) * nn,), generator=g, dtype=torch.int32).to(DEV)
    nsaved, nscr = lib.cpc_infonce_saved_bytes(b, t, k, dim, dim, nn), lib.cpc_infonce_scratch_bytes(b, t, k, dim, dim, nn)
    assert nsaved > 0 and nscr > 0
    csaved, cscr = torch.empty(nsaved, dtype=torch.uint8, device=DEV), torch.empty(nscr, dtype=torch.uint8, device=DEV)
    losses, acc = torch.full((k,), nan, device=DEV), torch.full((k,), nan, device=DEV)
    with pytest.raises(ValueError, match=f"holds {t - 1} frames"):
        _lib.check(lib.cpc_infonce_forward(_lib.ptr(c), _lib.ptr(zc), _lib.ptr(wpred), _lib.ptr(ext), None, _lib.ptr(losses), _lib.ptr(acc),
                                           _lib.ptr(csaved), _lib.ptr(cscr), b, t, t - 1, k, dim, dim, nn, st), "infonce_forward")
    # RNN: one layer, n = 2, t = 4 -- the cell has no deferred backward
    rn, rt = 2, 4
    rparams = [torch.zeros(s, device=DEV) for s in ((hidden, hidden), (hidden, hidden), (hidden,), (hidden,))]
    rx, dout = torch.zeros(rn, rt, hidden, device=DEV), torch.zeros(rn, rt, hidden, device=DEV)
    nsaved, nscr = lib.cpc_rnn_saved_bytes(rn, rt, hidden, hidden, 1), lib.cpc_rnn_scratch_bytes(rn, rt, hidden, hidden, 1)
    assert nsaved > 0 and nscr > 0
    rsaved, rscr = torch.zeros(nsaved, dtype=torch.uint8, device=DEV), torch.empty(nscr, dtype=torch.uint8, device=DEV)
    dx = torch.full_like(rx, nan)
    rgrads = [torch.full_like(p, nan) for p in rparams]
    calls = lib.cpc_recurrent_backward_calls()
    with pytest.raises(ValueError, match="RNN"):
        _lib.check(lib.cpc_rnn_backward(_lib.ptr(rx), _lib.ptr_array(rparams), _lib.ptr(dout), _lib.ptr(rsaved), _lib.ptr(rscr), _lib.ptr(dx),
                                        _lib.ptr_array(rgrads), rn, rt, hidden, hidden, 1, 1, st), "rnn_backward")
    assert lib.cpc_recurrent_backward_calls() == calls
    torch.cuda.synchronize()
    # nothing was launched: every output still holds its poison
    for out in [z, losses, acc, dx] + rgrads:
        assert bool(torch.isnan(out).all())


def test_train_step_with_signal_quality_files(tmp_path):
    """The feeder's third batch element (dataset.py:327-330) reaches the criterion's quality weighting
    (train.py:88-94,107; criterion.py:230,334-338): an epoch of trainStep on the fixture with generated estimate files."""
    import random
    from cpc2_amd import audio
    from cpc2_amd.dataset import AudioBatchData, filterSeqs, findAllSeqs
    from cpc2_amd.train import trainStep
    seq_names, speakers = findAllSeqs(GOLD_DB, extension=".flac")
    seq_names = filterSeqs(SEQ_LIST, seq_names)
    for i, (_spk, rel) in enumerate(seq_names):
        frames = audio.info(os.path.join(GOLD_DB, rel))[2] // 1600
        out = tmp_path / (os.path.splitext(rel)[0] + ".pt")
        out.parent.mkdir(parents=True, exist_ok=True)
        torch.save([torch.linspace(0.0, 30.0, frames).view(-1, 1), torch.linspace(50.0, 5.0, frames).view(-1, 1)], out)
    (tmp_path / "min_max.csv").write_text("min_snr,max_snr,min_c50,max_c50\n0,30,0,60\n")
    random.seed(0)
    data = AudioBatchData(GOLD_DB, 20480, seq_names, None, len(speakers), device=DEV, signal_quality_path=tmp_path,
                          signal_quality_mode="snr_c50")
    model, _ = _small_model(64)
    crit = cpc2_amd.CPCUnsupersivedCriterion(12, 64, 64, 32, rnnMode="linear", sizeInputSeq=128, growth_rate=2.0,
                                             inflection_point_x=0.4).to(DEV)
    crit.seed(3)
    opt = buildOptimizer(model, crit, lr=2e-4)
    loader = data.getDataLoader(8, "uniform", True)
    seq, label, quality = next(iter(loader))
    assert quality.is_cuda and quality.shape == (8, 12) and 0.0 <= float(quality.min()) and float(quality.max()) <= 1.0
    # weighted loss = weights (criterion.py:230) times the unweighted per-position losses, checked on one batch
    crit.seed(3)
    weighted, _ = crit(*model(seq[:, 0], label)[:2], label, quality)
    crit.seed(3)
    plain, _ = crit(*model(seq[:, 0], label)[:2], label, None)
    assert not torch.allclose(weighted, plain)
    logs = trainStep(loader, model, crit, opt, None, 1000)
    assert logs["iter"] >= 5 and np.isfinite(logs["locLoss_train"]).all()


# ----------------------------------------------------------------------------- criterion, inference-side API (g16)
@pytest.mark.parametrize("tag,mode", [("plain", None), ("reverse", "reverse")])
def test_get_prediction_cosine_sample_clean_vs_reference_golden(golden, tag, mode):
    """getPrediction / getCosineDistances / sampleClean of the reference (criterion.py:237-327) on the HIP kernels."""
    g = golden("g16_criterion_inference.npz")
    crit = make_criterion(4, 32, 32, 16, 50, mode=mode).eval()
    c = synth.features((4, 32, 32), 51).to(DEV)
    z = synth.features((4, 32, 32), 52, relu=True).to(DEV)
    torch.manual_seed(99)
    preds, label = crit.getPrediction(c, z, None)
    assert len(preds) == 4 and preds[0].shape == (4, 17, 28) and label.dtype == torch.long and label.shape == (4 * 28,)
    assert int(label.abs().sum()) == 0
    assert_close(torch.stack(preds), t(g[f"{tag}_pred"]), 2e-6, "getPrediction")
    # the CPU generator was advanced exactly as by the reference's call
    assert torch.equal(torch.randint(0, 1000, (4,)), t(g[f"{tag}_next_draws"]))
    state = torch.get_rng_state()
    cos = crit.getCosineDistances(c, z)
    assert torch.equal(torch.get_rng_state(), state), "getCosineDistances must not draw"
    assert cos[0].shape == (4, 1, 28)
    assert_close(torch.stack(cos), t(g[f"{tag}_cos"]), 2e-6, "getCosineDistances")
    torch.manual_seed(99)
    cands, lab2 = crit.sampleClean(z, 28)
    assert len(cands) == 4 and torch.equal(cands[0].cpu(), t(g[f"{tag}_cand_first"])) and torch.equal(cands[-1].cpu(), t(g[f"{tag}_cand_last"]))
    assert lab2.shape == (4 * 28,) and int(lab2.abs().sum()) == 0


def test_get_prediction_is_what_forward_scores():
    """CE of getPrediction's scores == forward()'s losses (same negatives), also with module predictors."""
    for rnn in ("linear", "transformer"):
        torch.manual_seed(3)
        crit = cpc2_amd.CPCUnsupersivedCriterion(4, 64, 64, 16, rnnMode=rnn, sizeInputSeq=32).to(DEV).eval()
        c = synth.features((3, 32, 64), 71).to(DEV)
        z = synth.features((3, 32, 64), 72, relu=True).to(DEV)
        crit.seed(11)
        losses, acc = crit(c, z, None)
        crit.seed(11)
        preds, label = crit.getPrediction(c, z, None)
        for k in range(4):
            lg = preds[k].permute(0, 2, 1).reshape(-1, 17)
            ce = torch.nn.functional.cross_entropy(lg, label)
            assert abs(float(ce) - float(losses[0, k])) <= 2e-5 * abs(float(ce)), (rnn, k)
            assert abs(float((lg.argmax(1) == 0).float().mean()) - float(acc[0, k])) <= 1.5 / lg.shape[0]


def test_cpc_module_matches_its_parts():
    """CPCModule (feature_loader.py:57-82) = model -> criterion scores -> softmax over the candidates."""
    from cpc2_amd.feature_loader import CPCModule
    model, _mp = _small_model()
    crit = make_criterion(12, 64, 64, 16, 23).eval()
    x = synth.audio_windows(2, 20480, 24)
    full = CPCModule(model.eval(), crit, main_distance_only=False, n_pred=-1)
    main = CPCModule(model.eval(), crit, main_distance_only=True, n_pred=2)
    assert full.getDownsamplingFactor() == 160
    crit.seed(5)
    probs = full((x, None))
    assert probs.shape == (2, 17, 116) and torch.allclose(probs.sum(1), torch.ones(2, 116, device=DEV), atol=1e-5)
    with torch.no_grad():
        cf, ef, _ = model(x.to(DEV), None)
    crit.seed(5)
    ref = torch.softmax(crit.getPrediction(cf, ef, None)[0][-1], dim=1)
    assert torch.equal(probs, ref)
    d = main((x, None))
    assert d.shape == (2, 1, 116) and torch.equal(d, crit.getCosineDistances(cf, ef)[2])
    # against the oracle: the positive's score of step 3
    p64 = to64(_mp)
    c64, z64 = O.model_forward(x.double(), p64)
    preds = [crit.wPrediction.predictors[i].weight.detach().double().cpu() for i in range(12)]
    want = O.prediction_scores(c64, z64, preds, None, 16)[2]
    assert_close(d, want, 5e-5, "main distance vs oracle")


def test_predictor_dropout_trains_and_is_off_in_eval():
    """dropout=True (criterion.py:113,168-169): nn.Dropout(0.5) on the predictions in training mode only."""
    crit = cpc2_amd.CPCUnsupersivedCriterion(4, 64, 64, 16, rnnMode="linear", dropout=True, sizeInputSeq=32).to(DEV)
    ref = cpc2_amd.CPCUnsupersivedCriterion(4, 64, 64, 16, rnnMode="linear", dropout=False, sizeInputSeq=32).to(DEV)
    ref.load_state_dict(crit.state_dict())
    assert isinstance(crit.wPrediction.dropout, torch.nn.Dropout) and crit.wPrediction.dropout.p == 0.5
    c = synth.features((3, 32, 64), 81).to(DEV).requires_grad_(True)
    z = synth.features((3, 32, 64), 82, relu=True).to(DEV).requires_grad_(True)
    crit.eval(); ref.eval()
    crit.seed(7); ref.seed(7)
    assert torch.equal(crit(c, z, None)[0], ref(c, z, None)[0])           # eval: identity
    crit.train()
    crit.seed(7)
    torch.manual_seed(0)
    la, _ = crit(c, z, None)
    la.sum().backward()
    assert torch.isfinite(la).all() and c.grad is not None and torch.isfinite(c.grad).all()
    g = [p.weight.grad for p in crit.wPrediction.predictors]
    assert all(x is not None and torch.isfinite(x).all() and float(x.abs().max()) > 0 for x in g)
    # the training-mode value is the no-dropout criterion applied to predictions masked by the same draw
    crit.seed(7)
    torch.manual_seed(0)
    cw = c[:, :28].detach()
    masked = [crit.wPrediction.dropout(torch.nn.functional.linear(cw, p.weight.detach())) for p in crit.wPrediction.predictors]
    from cpc2_amd.criterion import _InfoNCEPredFn
    ext = crit.sampleIndices(3, 32, 28, DEV)
    lb, _ = _InfoNCEPredFn.apply(z.detach(), ext, None, 16, *masked)
    assert_close(la.view(-1), lb.view(-1), 2e-5, "dropout path")


# ----------------------------------------------------------------------------- feature extraction (f3)
def test_build_feature_batch_and_streaming():
    """buildFeature_batch (feature_loader.py:370-433) == chunk-wise model calls; buildFeature streams a keepHidden model."""
    from cpc2_amd import audio
    from cpc2_amd.feature_loader import FeatureModule, buildFeature, buildFeature_batch
    model, mp = _small_model()
    path = os.path.join(GOLD_DB, "4397", "15668", "4397-15668-0003.flac")
    wav = audio.load(path)[0]
    n = wav.shape[1]
    fm = FeatureModule(model, False).eval()
    p64 = to64(mp)
    for strict in (False, True):
        got = buildFeature_batch(fm, path, strict=strict, maxSizeSeq=8000, batch_size=8)
        ref = []
        n_full = n // 8000
        for i in range(n_full):
            ref.append(O.model_forward(wav[:, i * 8000:(i + 1) * 8000].double().view(1, 1, -1), p64)[0])
        rest = n % 8000
        if rest >= 160:
            if strict:
                ref.append(O.model_forward(wav[:, -8000:].double().view(1, 1, -1), p64)[0][:, -(rest // 160):])
            else:
                ref.append(O.model_forward(wav[:, -rest:].double().view(1, 1, -1), p64)[0])
        ref = torch.cat(ref, dim=1)
        assert got.shape == ref.shape
        assert_close(got, ref, 5e-5, f"buildFeature_batch strict={strict}")
    # batch size does not matter; seqNorm normalises each chunk
    a = buildFeature_batch(fm, path, maxSizeSeq=8000, batch_size=3, seqNorm=True)
    b = buildFeature_batch(fm, path, maxSizeSeq=8000, batch_size=64, seqNorm=True)
    assert torch.allclose(a, b, atol=1e-5)
    assert float(a[:, :50].mean(dim=1).abs().max()) < 1e-4
    # keepHidden: chunked streaming through buildFeature == one pass over the whole file
    ks = cpc2_amd.CPCModel(cpc2_amd.CPCEncoder(64), cpc2_amd.CPCAR(64, 64, True, 1))
    ks.load_state_dict(mp)
    ks = ks.to(DEV).eval()
    whole_len = (n // 16000) * 16000                       # chunk borders on frame borders: the encoder sees the same frames
    streamed = buildFeature(FeatureModule(ks, False).eval(), wav[:, :whole_len], maxSizeSeq=16000)
    ks.gAR.hidden = None
    with torch.no_grad():
        z_chunks = [ks.gEncoder(wav[:, s:s + 16000].view(1, 1, -1).to(DEV)).permute(0, 2, 1) for s in range(0, whole_len, 16000)]
        ks.gAR.hidden = None
        whole = ks.gAR(torch.cat(z_chunks, dim=1)).cpu()
    assert streamed.shape == whole.shape
    assert_close(streamed, whole, 2e-5, "keepHidden streaming")


def test_reference_written_checkpoint_loads_into_hip_modules(golden):
    """tests/golden/ref_checkpoint was written by the reference's classes (tools/make_golden.py g17): loadModel builds the
    HIP modules from its args and weights; outputs match what the reference computed."""
    from cpc2_amd.feature_loader import getCheckpointData, loadModel
    g = golden("g17_ref_checkpoint_outputs.npz")
    run = os.path.join(os.path.dirname(GOLD_DB), "ref_checkpoint")
    path, logs, args = getCheckpointData(run)
    assert path.endswith("checkpoint_7.pt") and logs["epoch"] == [7] and args.hiddenEncoder == 32
    model, h_ar, h_enc = loadModel([path])
    assert (h_ar, h_enc) == (32, 32)
    model = model.to(DEV).eval()
    with torch.no_grad():
        c, z, _ = model(t(g["x"]).to(DEV), None)
    assert_close(z, t(g["z"]), 2e-5, "encoder of the reference checkpoint")
    assert_close(c, t(g["c"]), 5e-5, "context of the reference checkpoint")
    crit = cpc2_amd.CPCUnsupersivedCriterion(args.nPredicts, args.hiddenGar, args.hiddenEncoder, args.negativeSamplingExt,
                                             rnnMode=args.rnnMode, sizeInputSeq=args.sizeWindow // 160)
    crit.load_state_dict(torch.load(path, "cpu")["cpcCriterion"])


# ----------------------------------------------------------------------------- cooperative kernels fail loudly
@pytest.mark.parametrize("mode", ["GRU", "LSTM"])
def test_cooperative_recurrence_timeout_is_reported(monkeypatch, mode):
    """CPC_COOP_FAULT=1 makes member 0 of group 0 withhold one publish: its group's bounded waits run out, the outputs are
    poisoned with NaN AND the library reports it -- at cpc_async_error_check and at the next recurrent entry point."""
    lib = _lib.load()
    ar = cpc2_amd.CPCAR(256, 256, False, 1, mode=mode).to(DEV)
    x = synth.features((8, 6, 256), 5).to(DEV)
    stream = _lib.stream_ptr(DEV)
    _lib.check(lib.cpc_async_error_check(stream))                     # clean slate
    good = ar(x)
    _lib.check(lib.cpc_async_error_check(stream))
    assert torch.isfinite(good).all()
    monkeypatch.setenv("CPC_COOP_FAULT", "1")
    bad = ar(x)
    monkeypatch.delenv("CPC_COOP_FAULT")
    try:
        with pytest.raises(RuntimeError, match="gave up waiting"):
            _lib.check(lib.cpc_async_error_check(stream))
        assert torch.isnan(bad).any()
        _lib.check(lib.cpc_async_error_check(stream))                 # reported once, then cleared
        # the report switched the process to the streaming kernels (whatever kept the workgroups apart may still be there):
        # the next call works without anybody's help, and agrees with the cooperative kernels to rounding
        assert lib.cpc_coop_set_policy(-1) == 1
        launches = lib.cpc_coop_launches()
        streamed = ar(x)
        _lib.check(lib.cpc_async_error_check(stream))
        assert lib.cpc_coop_launches() == launches
        assert_close(streamed, good, 2e-6, "streaming kernel after the switch")
    finally:
        lib.cpc_coop_set_policy(0)
    # without an explicit check the NEXT call into the recurrent kernels reports it
    monkeypatch.setenv("CPC_COOP_FAULT", "1")
    ar(x)
    monkeypatch.delenv("CPC_COOP_FAULT")
    torch.cuda.synchronize()
    try:
        with pytest.raises(RuntimeError, match="gave up waiting"):
            ar(x)
    finally:
        lib.cpc_coop_set_policy(0)
    again = ar(x)
    _lib.check(lib.cpc_async_error_check(stream))
    assert torch.equal(again, good)


@pytest.mark.parametrize("mode", ["GRU", "LSTM"])
def test_cooperative_granule_epochs_across_launches_and_the_wrap(monkeypatch, mode):
    """The cooperative recurrent kernels exchange {epoch, value} granules through a buffer the library owns; every launch takes the
    next T + 1 epochs instead of clearing the buffer (coop.h, coop_comm_acquire).  Many launches in a row on one stream -- forward and
    backward, two layers, different window counts (different granule layouts over the same memory) -- give the results of a fresh
    process' first launch, bit for bit; and a buffer whose 32-bit epoch counter is about to wrap (CPC_COOP_EPOCH_START, read when a
    stream's buffer is created) clears itself once and goes on."""
    lib = _lib.load()
    ar = cpc2_amd.CPCAR(256, 256, False, 2, mode=mode).to(DEV)
    xs = [synth.features((n, 9, 256), 5 + n).to(DEV).requires_grad_(True) for n in (8, 3, 64, 8)]

    def run(x):
        x.grad = None
        out = ar(x)
        out.square().sum().backward()
        return out.detach().clone(), x.grad.clone()
    before = lib.cpc_coop_launches()
    first = [run(x) for x in xs]
    assert lib.cpc_coop_launches() - before == 4 * 2 * 2          # (4 inputs x 2 layers x forward + backward)
    for _rep in range(3):
        for x, (out, dx) in zip(xs, first):
            o2, d2 = run(x)
            assert torch.equal(o2, out) and torch.equal(d2, dx)
    assert torch.equal(first[0][0], first[3][0])                  # the same input after other shapes have used the buffer
    # a fresh stream = a fresh buffer, started 25 epochs below the wrap: T + 1 = 10 epochs per launch, four launches per run
    monkeypatch.setenv("CPC_COOP_EPOCH_START", str(0xFFFFFFF0 - 25))
    side = torch.cuda.Stream(torch.device(DEV))
    side.wait_stream(torch.cuda.current_stream(torch.device(DEV)))
    with torch.cuda.stream(side):
        for _rep in range(3):
            o2, d2 = run(xs[0])
            assert torch.equal(o2, first[0][0]) and torch.equal(d2, first[0][1])
    side.synchronize()
    _lib.check(lib.cpc_async_error_check(_lib.stream_ptr(torch.device(DEV))), "async error check")


def test_granule_buffers_of_abandoned_streams_are_given_back():
    """A recurrent launch takes its granule buffer by (device, stream); a process that makes a stream per request used to keep one
    buffer per stream it ever launched from (round-5 advice).  Thirty streams in a row: the results stay those of the first launch,
    bit for bit (a stream that comes back after its buffer was given away starts a fresh, zeroed one), and the library never holds
    more than eight buffers."""
    lib = _lib.load()
    ar = cpc2_amd.CPCAR(256, 256, False, 1).to(DEV)
    x = synth.features((8, 9, 256), 77).to(DEV)
    with torch.no_grad():
        ref = ar(x).clone()
    torch.cuda.synchronize()
    handles = set()
    for _sweep in range(2):
        for _i in range(30):
            side = torch.cuda.Stream(torch.device(DEV))
            handles.add(side.cuda_stream)
            side.wait_stream(torch.cuda.current_stream(torch.device(DEV)))
            with torch.cuda.stream(side), torch.no_grad():
                out = ar(x)
            side.synchronize()
            assert torch.equal(out, ref)
            assert 1 <= lib.cpc_coop_comm_buffers() <= 8
    assert len(handles) > 8                                            # (more distinct streams than buffers: some were given away)


def test_adam_leaves_non_finite_gradient_elements_alone_and_reports_them():
    """A NaN / inf gradient element (what a timed-out cooperative kernel leaves behind, on every rank after the all-reduce)
    must not reach the weights: parameter and moments of that element stay, the others step, and the asynchronous error
    check reports it (round-2 advice: the failure was loud but the weights were already poisoned)."""
    lib = _lib.load()
    stream = _lib.stream_ptr(DEV)
    _lib.check(lib.cpc_async_error_check(stream))                       # (clear anything an earlier test left)
    n = 5000
    p = torch.linspace(-1, 1, n, device=DEV)
    g = torch.full((n,), 0.5, device=DEV)
    g[7], g[4097] = float("nan"), float("inf")
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    p0 = p.clone()
    _lib.check(lib.cpc_adam_step(_lib.ptr(p), _lib.ptr(g), _lib.ptr(m), _lib.ptr(v), n, 1, 1e-2, 0.9, 0.999, 1e-8, 1.0, stream))
    with pytest.raises(RuntimeError, match="non-finite gradient"):
        _lib.check(lib.cpc_async_error_check(stream))
    bad = torch.tensor([7, 4097], device=DEV)
    assert torch.equal(p[bad], p0[bad]) and float(m[bad].abs().sum()) == 0 and float(v[bad].abs().sum()) == 0
    good = torch.ones(n, dtype=torch.bool, device=DEV)
    good[bad] = False
    assert torch.allclose(p[good], p0[good] - 1e-2, atol=1e-6) and torch.isfinite(p).all()
    _lib.check(lib.cpc_async_error_check(stream))                       # reported once, then clear


# ----------------------------------------------------------------------------- BASELINE configs at their real shapes
def _full_step_vs_oracle(hidden, layers, nneg, x, steps, lr, seed, tol_loss, tol_param):
    """`steps` Adam steps of the HIP path and of the fp32 CPU oracle on the same windows (reference semantics: 2b windows
    through encoder + GRU): loss per prediction step within tol_loss relative at every step, parameters after the last
    step within tol_param of their scale."""
    k = 12
    mp = synth.encoder_params(hidden, 31)
    mp.update(synth.gru_params(hidden, hidden, layers, 32))
    cp = synth.predictor_params(k, hidden, hidden, 33)
    model = cpc2_amd.CPCModel(cpc2_amd.CPCEncoder(hidden), cpc2_amd.CPCAR(hidden, hidden, False, layers))
    model.load_state_dict(mp)
    crit = cpc2_amd.CPCUnsupersivedCriterion(k, hidden, hidden, nneg, rnnMode="linear", sizeInputSeq=128)
    crit.load_state_dict(cp)
    model, crit = model.to(DEV), crit.to(DEV)
    opt = buildOptimizer(model, crit, lr=lr)
    crit.seed(seed)
    xd = x.to(DEV)
    label = torch.zeros(x.shape[0], dtype=torch.long, device=DEV)
    curve = []
    for _ in range(steps):
        tot, losses, _ = cpcStep(xd, xd, label, model, crit)
        tot.backward()
        opt.step()
        opt.zero_grad()
        curve.append(losses.detach().cpu())
    ref_curve, ref_params = O.train_steps(x, x, mp, cp, seed, steps, k, nneg, n_layers_gru=layers, lr=lr)
    for i in range(steps):
        err = float(((curve[i].view(-1) - ref_curve[i]).abs() / ref_curve[i].abs()).max())
        assert err <= tol_loss, f"step {i}: InfoNCE loss differs from the oracle by {err:.2e} relative"
    got = {n: p.detach().cpu() for n, p in list(crit.state_dict().items()) + list(model.state_dict().items())}
    # Adam moves every weight by about lr per step whatever the size of its gradient, so an element whose gradient is
    # rounding noise may legitimately end up 2 lr steps away: the bound below catches a missing or mis-scaled update,
    # the loss curve above is the tight check (step i + 1 sees step i's update)
    for n, ref in ref_params.items():
        d = float((got[n] - ref).abs().max())
        assert d <= 2.5 * lr * steps + tol_param * float(ref.abs().max()), f"{n}: {d:.2e}"
        moved = float((got[n] - (mp[n] if n in mp else cp[n])).abs().max())
        assert moved > 0.2 * lr, f"{n} was not updated"


def test_config_c5_cpc_large_full_step_vs_oracle():
    """BASELINE configs[4] per GPU at its real shapes -- hiddenEncoder = hiddenGar = 512, nLevelsGRU = 2, 256 negatives,
    nPredicts 12, 20480-sample windows -- at b = 2 (4 windows through the encoder): two steps against the oracle."""
    _full_step_vs_oracle(512, 2, 256, synth.audio_windows(2, 20480, 34), steps=2, lr=2e-4, seed=77, tol_loss=1e-3, tol_param=2e-3)


def test_config_c1_cpc_small_on_reference_test_data_vs_oracle():
    """BASELINE configs[0] at its real shapes: CPC-small (hidden 256, GRU, 12 predictions, 128 negatives) on windows of the
    reference's cpc/test_data fixture, batchSizeGPU = 8, three Adam steps against the CPU oracle."""
    import random
    random.seed(0)
    data = _feeder(DEV)
    seq, _label = next(iter(data.getDataLoader(8, "sequential", False)))
    _full_step_vs_oracle(256, 1, 128, seq[:, 0].cpu(), steps=3, lr=2e-4, seed=1234, tol_loss=1e-3, tol_param=2e-3)


@pytest.mark.parametrize("name,hidden,layers,ar", [("c2", 256, 1, "GRU"), ("c5", 512, 2, "GRU"), ("c4", 256, 1, "transformer")])
def test_full_batch_launch_geometry_vs_oracle_on_four_windows(name, hidden, layers, ar):
    """Round-4 review: at b = 64 (N = 128 windows: other tiles, K splits and windows-per-group choices than at b = 2) C4 / C5 were
    only compared with themselves.  Every op below the criterion is per window (model.py:102-108,188-207; transformers.py:52-70),
    so: the HIP model runs on all 128 windows, the fp64 oracle on windows {0, 63, 64, 127} alone -- z and c of those windows must
    agree (2e-5), and so must every parameter gradient of a loss that only involves those four windows (the oracle differentiated
    under the kernels' own ReLU decisions for them, read back from what the forward pass keeps: section 2 of DESIGN.md)."""
    n, sel = 128, [0, 63, 64, 127]
    model, mp = _full_size_model(hidden, layers, ar)
    x = synth.audio_windows(n, 20480, 33)
    xd = x.to(DEV)
    c, z, _ = model(xd, None)
    gc = synth.features((len(sel), 128, hidden), 34).to(DEV)
    gz = synth.features((len(sel), 128, hidden), 35).to(DEV)
    ((c[sel] * gc).sum() + (z[sel] * gz).sum()).backward()
    torch.cuda.synchronize()
    _lib.check(_lib.load().cpc_async_error_check(_lib.stream_ptr(torch.device(DEV))), "async error check")
    enc_params = {k: v for k, v in mp.items() if k.startswith("gEncoder.")}
    masks = _kernel_relu_decisions(hidden, enc_params, x, windows=sel)
    p64 = {k: v.double().requires_grad_(True) for k, v in mp.items()}
    pre = []
    z64 = O.encoder_forward(x[sel].double(), p64, "gEncoder.", masks=masks, pre_out=pre).permute(0, 2, 1)
    for i, (m, y) in enumerate(zip(masks, pre)):
        diff = m.bool() != (y > 0)                           # (a handful of pre-activations within fp32 rounding of zero)
        assert int(diff.sum()) <= max(2, int(1e-6 * diff.numel())), f"layer {i}: {int(diff.sum())} ReLU decisions differ from the fp64 oracle's"
        if diff.any():
            assert float(y[diff].abs().max() / y.abs().max()) <= 1e-5
    if ar == "transformer":
        c64 = z64
        for layer in range(layers):
            c64 = O.transformer_layer_forward(c64, p64, f"gAR.{layer}.")
    else:
        c64, _ = O.gru_forward(z64, p64, layers, "gAR.baseNet.")
    assert_close(z[sel], z64, 2e-5, "z of the four windows")
    assert_close(c[sel], c64, 2e-5, "c of the four windows")
    ((c64 * gc.cpu().double()).sum() + (z64 * gz.cpu().double()).sum()).backward()
    worst = 0.0
    for pname, p in model.named_parameters():
        ref = p64[pname].grad
        worst = max(worst, rel_err(p.grad, ref))
        assert_close(p.grad, ref, 2e-4, f"grad {pname}")
    print(f"{name}: four-window gradients at N = {n}: worst {worst:.2e} of scale")


def test_library_streams_run_beside_the_training_stream():
    """A HIP stream is served by one of a few hardware queues, assigned by use count when it is created; two streams on one queue
    run one after the other.  In a process crowded with streams (a process group's pools) the library's side stream used to land,
    now and then, on the training stream's queue (round 5's +1 ms per step).  cpc_stream_create_apart tests its candidates: here
    in a process that first creates forty streams, against the current stream, and the test itself is shown to tell a shared
    queue from a separate one."""
    lib = _lib.load()
    crowd = [torch.cuda.Stream(DEV) for _ in range(40)]
    cur = _lib.stream_ptr(torch.device(DEV))
    verdicts = [lib.cpc_streams_overlap(cur, ctypes.c_void_p(s.cuda_stream)) for s in crowd[:16]]
    assert all(v in (0, 1) for v in verdicts), verdicts
    assert 0 in verdicts and 1 in verdicts, f"sixteen plain streams over the default hardware queues: {verdicts}"
    for _ in range(6):                                       # (more than there are queues: each is apart from the CALLER's)
        raw = ctypes.c_void_p()
        avoid = (ctypes.c_void_p * 1)(cur.value)
        _lib.check(lib.cpc_stream_create_apart(avoid, 1, ctypes.byref(raw)), "stream_create_apart")
        assert lib.cpc_streams_overlap(cur, raw) == 1
    side = ctypes.c_void_p()
    _lib.check(lib.cpc_side_stream(cur, ctypes.byref(side)), "side_stream")
    assert lib.cpc_streams_overlap(cur, side) == 1
    assert lib.cpc_stream_apart_failures() == 0
    torch.cuda.synchronize()
    del crowd


def test_prefetched_indices_outlive_the_staging_ring():
    """With `prefetch` the sampler's worker rewrites one of RING persistent device buffers RING - 1 calls after it was filled.
    What sample() hands out is a copy: indices kept across more than 2 * RING later calls (saved for a late backward, logged) still
    equal the host sampler's -- and with `alias_ring` (the opt-in) they demonstrably do not."""
    b, t_len, k, nn = 4, 64, 12, 32
    ref, dev, alias = (cpc2_amd.criterion.NegativeSampler() for _ in range(3))
    for smp in (ref, dev, alias):
        smp.seed(9)
    dev.prefetch = alias.prefetch = True
    alias.alias_ring = True
    n = 2 * cpc2_amd.criterion.NegativeSampler.RING + 3
    want = [ref.sample_host(b, t_len, t_len - k, nn, time_major=True).clone() for _ in range(n)]
    kept = [dev.sample(b, t_len, t_len - k, nn, torch.device(DEV)) for _ in range(n)]
    kept_alias = [alias.sample(b, t_len, t_len - k, nn, torch.device(DEV)) for _ in range(n)]
    torch.cuda.synchronize()
    assert all(torch.equal(g.cpu(), w) for g, w in zip(kept, want))
    assert torch.equal(kept_alias[-1].cpu(), want[-1])
    assert not all(torch.equal(g.cpu(), w) for g, w in zip(kept_alias, want)), "the ring was expected to have wrapped"


def test_a_gradient_home_serves_one_consumer():
    """split_windows tags its parts with a fixed place in the encoder output's gradient buffer; the first function that consumes a
    part writes there in place.  A SECOND consumer of the same part (a subclass that runs two recurrent nets on x) must get a buffer
    of its own -- both writing the home would make autograd add the buffer to itself."""
    from cpc2_amd._route import split_windows
    hidden, n, t_len = 256, 6, 32
    torch.manual_seed(2)
    ar1 = cpc2_amd.CPCAR(hidden, hidden, False, 1).to(DEV)
    ar2 = cpc2_amd.CPCAR(hidden, hidden, False, 1).to(DEV)
    x = torch.randn(n, t_len, hidden, device=DEV)
    gout = torch.randn(n // 2, t_len, hidden, device=DEV)

    def run(tagged):
        xin = x.clone().requires_grad_(True)
        first = split_windows(xin, n // 2)[0] if tagged else xin[:n // 2]
        out = ar1(first) + 2.0 * ar2(first)
        (out * gout).sum().backward()
        return xin.grad.clone()
    plain, tagged = run(False), run(True)
    assert float(plain[n // 2:].abs().max()) == 0.0 and float(tagged[n // 2:].abs().max()) == 0.0
    assert_close(tagged[:n // 2], plain[:n // 2], 2e-6, "gradient of a part with two consumers")


def test_a_first_windows_home_serves_one_consumer():
    """The same for first_windows, whose home the criterion's backward honours for dc: the loss is the sum of TWO criterion calls on
    one first_windows output (different negatives).  Only the first may write dc into the cached buffer; the gradient equals that of
    the plain slice c_full[:2], the windows 2.. stay exactly zero, and a second pass reuses the buffer with the same result."""
    from cpc2_amd import _route
    torch.manual_seed(4)
    crit = cpc2_amd.CPCUnsupersivedCriterion(4, 32, 32, 8, rnnMode="linear", sizeInputSeq=16).to(DEV)
    c_data = torch.randn(4, 16, 32, device=DEV)
    z = torch.randn(2, 16, 32, device=DEV)
    label = torch.zeros(2, dtype=torch.long, device=DEV)

    def run(tagged):
        crit.seed(11)
        crit.zero_grad()
        c_full = c_data.clone().requires_grad_(True)
        c = _route.first_windows(c_full, 2) if tagged else c_full[:2]
        (crit(c, z, label)[0].sum() + crit(c, z, label)[0].sum()).backward()
        return c_full.grad.clone()
    plain, tagged = run(False), run(True)
    buf = _route.cached_grad_buffer((4, 16, 32), c_data.device, ("context", 2))
    again = run(True)
    assert _route.cached_grad_buffer((4, 16, 32), c_data.device, ("context", 2)) is buf, "the cached buffer was not reused"
    assert float(plain[:2].abs().max()) > 0
    for name, got in (("tagged", tagged), ("tagged, second pass", again)):
        assert float(plain[2:].abs().max()) == 0.0 and float(got[2:].abs().max()) == 0.0, name
        assert_close(got[:2], plain[:2], 2e-6, f"gradient of a first_windows output with two consumers ({name})")
    assert_close(again, tagged, 2e-6, "gradient of the second pass through the cached buffer")


def test_forward_hooks_keep_the_reference_call():
    """cpcStep's default form calls the encoder and the context network directly; a forward hook on the model or the encoder would then
    never fire.  With a hook registered the step goes through CPCModel.__call__ (the reference's own call) -- same losses."""
    model, crit = _step_model(256, 1, "GRU", 32)
    x = synth.audio_windows(4, 20480, 31).to(DEV)
    label = torch.zeros(4, dtype=torch.long, device=DEV)
    crit.seed(3)
    _tot, base, _ = cpcStep(x, x, label, model, crit)
    fired = []
    handle = model.gEncoder.register_forward_hook(lambda mod, inp, out: fired.append(tuple(out.shape)))
    crit.seed(3)
    _tot, hooked, _ = cpcStep(x, x, label, model, crit)
    handle.remove()
    assert fired == [(8, 256, 128)], fired
    assert_close(hooked, base, 1e-6, "losses with a forward hook on the encoder")


def test_prefetch_with_changing_batch_sizes_is_bit_exact():
    """The same-speaker sampler ends every speaker with a partial batch: the call after a draw ahead then has another size.  The
    generator is rewound to where it stood before that draw, so the sequence of index tensors equals the host sampler's (= the
    reference's torch.randint calls, golden g1) whatever the sizes do."""
    t_len, k, nn = 64, 12, 32
    # smaller calls after a draw ahead for the full batch (a prefix of its words), runs of them, a LARGER call (the draw is undone),
    # a host-side call in between, prefetch switched off behind a smaller call
    sizes = [8, 8, 5, 8, 8, 8, 3, 3, 8, 8, 12, 12, 5, 12, 8, 7, 8, "host", 8, 5, "off", 8, 8, "on"] + [2] * 12 + [12, 2, 2, 12]
    ref, dev = cpc2_amd.criterion.NegativeSampler(), cpc2_amd.criterion.NegativeSampler()
    ref.prefetch = False
    ref.seed(21)
    dev.seed(21)
    dev.prefetch = True
    for i, b in enumerate(sizes):
        if b == "host":
            assert torch.equal(dev.sample_host(6, t_len, t_len - k, nn, time_major=True), ref.sample_host(6, t_len, t_len - k, nn, time_major=True))
            continue
        if b in ("off", "on"):
            dev.prefetch = b == "on"
            continue
        want = ref.sample_host(b, t_len, t_len - k, nn, time_major=True)
        got = dev.sample(b, t_len, t_len - k, nn, torch.device(DEV))
        assert torch.equal(got.cpu(), want), (i, b)


def test_prefetch_under_torchs_global_generator_is_bit_exact():
    """The module's default takes the negatives from torch's global CPU generator (the reference's torch.randint calls).  With
    `prefetch` the next call's words are drawn ahead from the state the sampler left in torch -- valid only while nobody else
    uses that generator: a torch.rand in between, a host-side call or another batch size undo the draw.  Index tensors AND the
    generator's state after every call equal the plain path's."""
    t_len, k, nn = 64, 12, 32
    plan = [(8, None), (8, None), (8, "rand"), (5, None), (8, None), (8, "host"), (8, None), (8, None)]
    results = []
    for prefetch in (False, True):
        smp = cpc2_amd.criterion.NegativeSampler()
        smp.prefetch = prefetch
        torch.manual_seed(77)
        seen = []
        for b, between in plan:
            got = smp.sample(b, t_len, t_len - k, nn, torch.device(DEV)).cpu()
            seen.append((got, torch.get_rng_state().clone()))
            if between == "rand":
                torch.rand(3)                                   # someone else consumes torch's stream
            elif between == "host":
                seen.append((smp.sample_host(b, t_len, t_len - k, nn, time_major=True).clone(), torch.get_rng_state().clone()))
        results.append(seen)
    assert len(results[0]) == len(results[1])
    for i, ((a, sa), (c, sc)) in enumerate(zip(*results)):
        assert torch.equal(a, c), f"call {i}: indices differ with prefetch"
        assert torch.equal(sa, sc), f"call {i}: torch's generator state differs with prefetch"



def test_prefetch_serves_calls_by_the_fast_paths():
    """The bit-exact tests above pass just as well when every call takes the slow path; `served` tells.  By the rules of
    NegativeSampler.sample: the draws ahead are made for the largest call seen, so on a private stream the first call and a LARGER
    one draw for themselves, the call drawn for is served ahead and a smaller one from a prefix of the words on the device;
    under torch's generator a smaller call draws for itself (no prefix there) and the draws ahead stay with the large size."""
    t_len, k, nn = 64, 12, 32
    plans = [(False, [8, 8, 5, 8, 3, 3, 8, 12, 12], ["drawn", "ahead", "prefix", "ahead", "prefix", "prefix", "ahead", "drawn", "ahead"]),
             (True, [8, 8, 5, 8], ["drawn", "ahead", "drawn", "ahead"])]
    for follow_torch, sizes, want_served in plans:
        ref, dev = cpc2_amd.criterion.NegativeSampler(), cpc2_amd.criterion.NegativeSampler()
        if follow_torch:
            torch.manual_seed(33)
        else:
            ref.seed(33)
            dev.seed(33)
        want = [ref.sample_host(b, t_len, t_len - k, nn, time_major=True).clone() for b in sizes]
        if follow_torch:
            torch.manual_seed(33)
        assert dev.prefetch and dev.follow_torch == follow_torch and not dev.served
        served = []
        for i, b in enumerate(sizes):
            before = dev.served.copy()
            got = dev.sample(b, t_len, t_len - k, nn, torch.device(DEV))
            assert torch.equal(got.cpu(), want[i]), (follow_torch, i, b)
            served += list((dev.served - before).elements())
        assert served == want_served, (follow_torch, served)
