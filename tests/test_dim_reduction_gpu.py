"""cpc_seq_moments_accumulate / cpc_center_scale_rows (csrc/seqmoments.hip) and cpc2_amd.dim_reduction on the GPU: the moments
exactly on integer data with NaN wherever the kernel must not read, the f64 difference, the f64 sum bounds on data with an
offset, bits and running totals; the centring exactly against float32 numpy; PCA / SFALinear fitted on the golden inputs against
the reference's recorded fit (g29); both forwards against their float64 statement and the recorded outputs; and the two tools end
to end into eval_ABX from_pre_computed."""
import json
import os
import random
from fractions import Fraction

import numpy as np
import pytest
import torch

import dim_reduction_oracle as DO
from cpc2_amd import _lib
from cpc2_amd import dim_reduction as DR
from cpc2_amd._lib import check, ptr, scratch, stream_ptr
from cpc2_amd.eval import build_reduced_features as BR
from cpc2_amd.eval import eval_ABX

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DB = os.path.join(GOLDEN, "test_db")
CKPT = os.path.join(GOLDEN, "ref_checkpoint", "checkpoint_7.pt")
DEV = torch.device("cuda:0")
PCA_BUFFERS = ("var", "mean", "PCA_mul", "PCA_values")
SFA_BUFFERS = ("covar_speed", "mean_x", "square_x", "covar_x", "normalizer", "PCA_mul", "PCA_values", "projection")
CASES = [("k8", 3, 16, 8), ("k64", 6, 40, 64)]

SHAPES = [(1, 2, 0, 1), (1, 2, 1, 3), (3, 5, 1, 5), (2, 33, 0, 63), (2, 31, 3, 64), (4, 32, 1, 65), (7, 587, 1, 48),
          (3, 130, 1, 512), (5, 128, 1, 256)]


@pytest.fixture(scope="module")
def g29():
    with np.load(os.path.join(GOLDEN, "g29_dim_reduction.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


# --------------------------------------------------------------------------- cpc_seq_moments_accumulate
def _accumulate(xd, ld, seq_stride, b, s, skip, d, sums, gram, dgram):
    lib = _lib.load()
    nb = lib.cpc_seq_moments_scratch_bytes(b, s, skip, d)
    assert nb > 0
    check(lib.cpc_seq_moments_accumulate(ptr(xd), ld, seq_stride, b, s, skip, d, ptr(sums), ptr(gram), ptr(dgram),
                                         ptr(scratch(nb, DEV)), nb, stream_ptr(DEV)), "seq_moments_accumulate")


def _fresh(d):
    return (torch.zeros(d, dtype=torch.float64, device=DEV), torch.zeros(d, d, dtype=torch.float64, device=DEV),
            torch.zeros(d, d, dtype=torch.float64, device=DEV))


def _strided(x, skip, pad_cols=3, gap=5):
    """x [b, s, d] float32 -> (flat host buffer, ld, seq_stride) with ld > d and seq_stride > s * ld, NaN in the skipped frames,
    the padding columns and the gap behind every sequence."""
    b, s, d = x.shape
    ld = d + pad_cols
    seq_stride = s * ld + gap
    buf = np.full((b, seq_stride), np.nan, np.float32)
    view = buf[:, :s * ld].reshape(b, s, ld)
    view[:, skip:, :d] = x[:, skip:]
    return buf.reshape(-1), ld, seq_stride


def _run(x, skip, strided=True, totals=None):
    b, s, d = x.shape
    if strided:
        flat, ld, seq_stride = _strided(x, skip)
    else:
        flat, ld, seq_stride = np.ascontiguousarray(x).reshape(-1), d, s * d
    sums, gram, dgram = _fresh(d) if totals is None else totals
    _accumulate(torch.from_numpy(flat).to(DEV), ld, seq_stride, b, s, skip, d, sums, gram, dgram)
    return sums.cpu().numpy(), gram.cpu().numpy(), dgram.cpu().numpy()


@pytest.mark.parametrize("b,s,skip,d", SHAPES)
def test_integer_inputs_give_the_exact_moments(b, s, skip, d):
    """Integers in [-64, 64]: every difference, product and partial sum is an exact f64 integer, so sums, gram and dgram must EQUAL
    int64 numpy whatever the order of summation.  ld > d, seq_stride > s * ld, and NaN sits in the skipped frames, the padding
    columns and the gap: one read of any of them shows."""
    rng = np.random.default_rng(1000 * s + d)
    xi = rng.integers(-64, 65, size=(b, s, d), dtype=np.int64)
    ref_s, ref_g, ref_d = DO.seq_moments_int(xi, skip)
    before = rng.integers(-5, 6, size=(d, d))
    before = (before + before.T).astype(np.float64)                       # what dgram (a running, symmetric total) holds already
    totals = _fresh(d)
    totals[2].copy_(torch.from_numpy(before))
    sums, gram, dgram = _run(xi.astype(np.float32), skip, totals=totals)
    assert np.array_equal(sums, ref_s.astype(np.float64))
    assert np.array_equal(gram, ref_g.astype(np.float64)) and np.array_equal(gram, gram.T)
    if s - skip == 1:
        assert not ref_d.any() and np.array_equal(dgram, before)            # no difference: dgram is left as it was
    else:
        assert np.array_equal(dgram - before, ref_d.astype(np.float64))
        assert np.array_equal(dgram - before, (dgram - before).T)


def test_the_difference_is_taken_in_f64():
    """A window alternating 16777216 and 0.5: every difference is +-16777215.5 in f64 and +-16777216 in f32.  dgram must equal
    16777215.5^2 times the pair count exactly (7 pairs: every partial sum has at most 53 bits)."""
    s, d = 8, 3
    x = np.zeros((1, s, d), np.float32)
    x[0, 0::2] = 16777216.0
    x[0, 1::2] = 0.5
    _, gram, dgram = _run(x, 0)
    want = Fraction(16777215.5) ** 2 * (s - 1)
    assert Fraction(float(want)) == want and float(want) != 16777216.0 ** 2 * (s - 1)
    assert np.array_equal(dgram, np.full((d, d), float(want)))
    level = Fraction(16777216) ** 2 * 4 + Fraction(1, 4) * 4
    assert Fraction(float(level)) == level and np.array_equal(gram, np.full((d, d), float(level)))


@pytest.mark.parametrize("b,s,skip,d", [(5, 257, 1, 48), (3, 100, 2, 200), (2, 1031, 0, 65)])
def test_offset_inputs_within_the_f64_sum_bounds(b, s, skip, d):
    """randn + 1000: gram and sums within cca_oracle.moments_bound of the kept rows, dgram within (2 n + 4) 2^-53 |D|^T |D|."""
    rng = np.random.default_rng(b * s + d)
    x = (rng.standard_normal((b, s, d)) + 1000.0).astype(np.float32)
    sums, gram, dgram = _run(x, skip)
    ref_s, ref_g, ref_d = DO.seq_moments(x, skip)
    bs, bg = DO.level_bound(x, skip)
    bd = DO.diff_bound(x, skip)
    print("gram error / bound", (np.abs(gram - ref_g) / bg).max(), "sums", (np.abs(sums - ref_s) / bs).max(),
          "dgram", (np.abs(dgram - ref_d) / bd).max())
    assert (np.abs(gram - ref_g) <= bg).all() and (np.abs(sums - ref_s) <= bs).all()
    assert (np.abs(dgram - ref_d) <= bd).all()
    assert np.array_equal(gram, gram.T) and np.array_equal(dgram, dgram.T)


def test_wide_range_inputs_within_the_f64_sum_bounds():
    """randn + 1000 lies on a grid of 2^-14, where the sums and the products of differences happen to be exact.  Here every
    element has a magnitude of its own over six decades, so every sum rounds: the same bounds."""
    b, s, skip, d = 4, 300, 1, 70
    rng = np.random.default_rng(77)
    x = (rng.standard_normal((b, s, d)) * 10.0 ** rng.uniform(-3.0, 3.0, size=(b, s, d))).astype(np.float32)
    sums, gram, dgram = _run(x, skip)
    ref_s, ref_g, ref_d = DO.seq_moments(x, skip)
    bs, bg = DO.level_bound(x, skip)
    bd = DO.diff_bound(x, skip)
    print("gram error / bound", (np.abs(gram - ref_g) / bg).max(), "sums", (np.abs(sums - ref_s) / bs).max(),
          "dgram", (np.abs(dgram - ref_d) / bd).max())
    assert (np.abs(gram - ref_g) <= bg).all() and (np.abs(sums - ref_s) <= bs).all() and (np.abs(dgram - ref_d) <= bd).all()


def test_same_bits_running_totals_and_equal_triangles():
    b, s, skip, d = 6, 200, 1, 70
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((b, s, d)) + 1000.0).astype(np.float32)
    one = _run(x, skip)
    again = _run(x, skip)
    for a, c in zip(one, again):
        assert np.array_equal(a, c)                                       # the same call, the same bits

    def halves():
        totals = _fresh(d)
        _run(x[:b // 2], skip, totals=totals)
        return _run(x[b // 2:], skip, totals=totals)

    h1, h2 = halves(), halves()
    for a, c in zip(h1, h2):
        assert np.array_equal(a, c)
    bs, bg = DO.level_bound(x, skip)
    bd = DO.diff_bound(x, skip)
    assert (np.abs(h1[0] - one[0]) <= bs).all() and (np.abs(h1[1] - one[1]) <= bg).all() and (np.abs(h1[2] - one[2]) <= bd).all()
    ref = DO.seq_moments(x, skip)
    assert (np.abs(h1[1] - ref[1]) <= bg).all() and (np.abs(h1[2] - ref[2]) <= bd).all()
    for m in (one[1], one[2], h1[1], h1[2]):
        assert np.array_equal(m, m.T)
    # contiguous rows give the bits of the strided call
    for a, c in zip(one, _run(x, skip, strided=False)):
        assert np.array_equal(a, c)


# --------------------------------------------------------------------------- cpc_center_scale_rows
@pytest.mark.parametrize("n", [1, 257, 4099])
@pytest.mark.parametrize("d", [1, 63, 512])
def test_center_scale_rows_equals_float32_numpy(n, d):
    """(x - mean) / (scale + float32(1e-8)), each operation rounded once: with strides, with and without scale, and in place."""
    lib = _lib.load()
    rng = np.random.default_rng(n + d)
    ldx, ldy = d + 2, d + 5
    xb = (3.0 * rng.standard_normal((n, ldx)) + 1.0).astype(np.float32)
    mean = rng.standard_normal(d).astype(np.float32)
    scale = (np.abs(rng.standard_normal(d)) + 0.1).astype(np.float32)
    scale[0] = 0.0                                                        # the constant alone divides
    xd, md, sd = (torch.from_numpy(a).to(DEV) for a in (xb, mean, scale))
    for sc_host, sc_dev in ((scale, sd), (None, None)):
        want = DO.center_scale_f32(xb[:, :d], mean, sc_host)
        yd = torch.full((n, ldy), 7.0, dtype=torch.float32, device=DEV)
        check(lib.cpc_center_scale_rows(ptr(xd), ldx, ptr(md), ptr(sc_dev), ptr(yd), ldy, n, d, stream_ptr(DEV)), "center_scale_rows")
        y = yd.cpu().numpy()
        assert np.array_equal(y[:, :d], want) and (y[:, d:] == 7.0).all()
        assert np.array_equal(xd.cpu().numpy(), xb)                       # the input is left as it was
        inplace = xd.clone()
        check(lib.cpc_center_scale_rows(ptr(inplace), ldx, ptr(md), ptr(sc_dev), ptr(inplace), ldx, n, d, stream_ptr(DEV)),
              "center_scale_rows")
        got = inplace.cpu().numpy()
        assert np.array_equal(got[:, :d], want) and np.array_equal(got[:, d:], xb[:, d:])


# --------------------------------------------------------------------------- the fit
def _relative(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _fitted(g, tag, kind, exact_counts=False):
    x = torch.from_numpy(g[f"{tag}_x"]).to(DEV)
    k = x.size(2)
    module = (DR.PCA(k) if kind == "pca" else DR.SFALinear(k, exact_counts=exact_counts)).to(DEV)
    half = x.size(0) // 2                                                 # two updates: the totals run on
    module.update(x[:half])
    module.update(x[half:])
    return module


@pytest.mark.parametrize("tag,b,s,k", CASES)
def test_fit_reproduces_the_reference(g29, tag, b, s, k):
    """The f64 totals EQUAL the reference's recorded raw sums (the golden inputs lie on a grid of 2^-10: every sum is exact), the
    counts are the reference's, and the built f32 buffers are within 1e-6 of the recorded float64 ones, relative to each buffer's
    largest magnitude, eigenvector rows compared after the sign rule."""
    pca = _fitted(g29, tag, "pca")
    sx, sxx = pca.totals()
    assert pca.N == int(g29[f"{tag}_pca_N"])
    assert np.array_equal(sx, g29[f"{tag}_pca_raw_mean"]) and np.array_equal(sxx, g29[f"{tag}_pca_raw_var"])
    pca.build()
    sfa = _fitted(g29, tag, "sfa")
    sums, gram, dgram = sfa.totals()
    assert (sfa.N_x, sfa.N_speed) == (int(g29[f"{tag}_sfa_N_x"]), int(g29[f"{tag}_sfa_N_speed"]))
    assert (sfa.rows_summed, sfa.differences_summed) == DO.counts(b, s, exact=True)
    assert np.array_equal(sums, g29[f"{tag}_sfa_raw_mean_x"]) and np.array_equal(gram, g29[f"{tag}_sfa_raw_covar_x"])
    assert np.array_equal(dgram, g29[f"{tag}_sfa_raw_covar_speed"])
    sfa.build()
    assert not pca.building and not sfa.building
    for module, prefix, names in ((pca, "pca", PCA_BUFFERS), (sfa, "sfa", SFA_BUFFERS)):
        assert tuple(module.state_dict()) == names
        for name in names:
            got, ref = module.state_dict()[name], g29[f"{tag}_{prefix}_{name}"]
            assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == ref.shape
            got = got.double().cpu().numpy()
            if name in ("PCA_mul", "projection"):
                got, ref = DO.sign_rule(got[0]), DO.sign_rule(ref[0])
                assert np.array_equal(got, module.state_dict()[name][0].double().cpu().numpy())      # the module signs its rows
            dev = _relative(got, ref)
            print(tag, prefix, name, "relative distance", dev)
            assert dev <= 1e-6
    # exact counts: the mean is s / (s - 1) of the default's
    exact = _fitted(g29, tag, "sfa", exact_counts=True)
    exact.build()
    assert np.allclose(exact.solution["mean_x"], sfa.solution["mean_x"] * s / (s - 1), rtol=8 * DO.U53, atol=0)


# --------------------------------------------------------------------------- the forwards
def _reference_module(g, tag, kind):
    """The module loaded from a state dict written as the reference writes it: the recorded float64 buffers as float32."""
    names = PCA_BUFFERS if kind == "pca" else SFA_BUFFERS
    k = g[f"{tag}_x"].shape[2]
    module = DR.PCA(k) if kind == "pca" else DR.SFALinear(k)
    module.load_state_dict({n: torch.from_numpy(g[f"{tag}_{kind}_{n}"]).float() for n in names})
    module.building = False
    return module.to(DEV)


def _held_to_statement(module, x, tag):
    """module(x) against the float64 statement from the module's own (f32) buffers, within forward_bound."""
    before = x.clone()
    y = module(x)
    assert torch.equal(x, before)                                          # forward never touches its input
    buffers = {n: v.double().cpu().numpy() for n, v in module.state_dict().items()}
    xh = x.cpu().numpy()
    k = xh.shape[-1]
    if isinstance(module, DR.PCA):
        ref = DO.pca_forward(buffers, xh)
        xc = xh.astype(np.float64).reshape(-1, k) - buffers["mean"]
        bound = DO.forward_bound(buffers["PCA_mul"][0], xc, roundings=1)
    else:
        ref = DO.sfa_forward(buffers, xh)
        xc = (xh.astype(np.float64).reshape(-1, k) - buffers["mean_x"]) / (buffers["square_x"] + 1e-08)
        proj, norm = buffers["projection"][0], buffers["normalizer"][0]
        bound = DO.forward_bound(proj @ norm, xc, roundings=3)
        bound = bound + 2.0 * k * DO.U53 * (np.abs(xc) @ (np.abs(proj) @ np.abs(norm)).T)      # the statement's two f64 products
    got = y.double().cpu().numpy()
    assert got.shape == ref.shape and y.dtype == torch.float32 and y.is_cuda
    ratio = float((np.abs(got - ref).reshape(bound.shape) / bound).max())
    print(tag, type(module).__name__, tuple(xh.shape), "->", got.shape, "worst |y - y64| / bound", ratio)
    assert ratio <= 1.0
    return got


@pytest.mark.parametrize("tag,b,s,k", CASES)
def test_forward_against_the_statement_and_the_recorded_outputs(g29, tag, b, s, k):
    held = torch.from_numpy(g29[f"{tag}_held_out"]).to(DEV)
    wide = torch.from_numpy(np.concatenate([g29[f"{tag}_held_out"]] * 2, axis=2)).to(DEV)
    for kind in ("pca", "sfa"):
        module = _reference_module(g29, tag, kind)
        recorded = {n: g29[f"{tag}_{kind}_{n}"] for n in (PCA_BUFFERS if kind == "pca" else SFA_BUFFERS)}
        y3 = _held_to_statement(module, held, tag)                                            # [b, s, k]
        y2 = _held_to_statement(module, held.view(-1, k), tag)                                # [n, k]
        assert y3.shape == (2, s, k) and y2.shape == (2 * s, k) and np.array_equal(y3.reshape(-1, k), y2)
        ys = _held_to_statement(module, wide[:, :, :k], tag)                                  # rows with a stride
        assert np.array_equal(ys, y3)
        # the recorded float64 forward: within the f32 storage of the buffers plus the device's bound
        ref = g29[f"{tag}_{kind}_forward"]
        xh = g29[f"{tag}_held_out"]
        if kind == "pca":
            xc = xh.astype(np.float64).reshape(-1, k) - recorded["mean"]
            bound = DO.pca_storage_bound(recorded, xh) + DO.forward_bound(recorded["PCA_mul"][0], xc, 1).reshape(ref.shape)
        else:
            xc = (xh.astype(np.float64).reshape(-1, k) - recorded["mean_x"]) / (recorded["square_x"] + 1e-08)
            both = np.abs(recorded["projection"][0]) @ np.abs(recorded["normalizer"][0])
            bound = DO.sfa_storage_bound(recorded, xh) + DO.forward_bound(both, xc, 3).reshape(ref.shape)
        ratio = float((np.abs(y3 - ref) / bound).max())
        print(tag, kind, "against the recorded forward: worst / bound", ratio, "relative", _relative(y3, ref))
        assert ratio <= 1.0
    # after selectDimensions: the reference's selection, the recorded output, and a new folded matrix
    sfa = _reference_module(g29, tag, "sfa")
    full = sfa(held)
    select = torch.from_numpy(g29[f"{tag}_sfa_select"])
    sfa.selectDimensions(select)
    assert tuple(sfa.projection.shape) == (1, k // 2, k)
    cut = _held_to_statement(sfa, held, tag)
    assert cut.shape == (2, s, k // 2)
    _held_to_statement(sfa, held.view(-1, k), tag)
    recorded = {n: g29[f"{tag}_sfa_{n}"] for n in SFA_BUFFERS}
    proj = recorded["PCA_mul"][:, g29[f"{tag}_sfa_select"] > 0]
    xc = (g29[f"{tag}_held_out"].astype(np.float64).reshape(-1, k) - recorded["mean_x"]) / (recorded["square_x"] + 1e-08)
    ref = g29[f"{tag}_sfa_forward_selected"]
    bound = DO.sfa_storage_bound(recorded, g29[f"{tag}_held_out"], proj) + \
        DO.forward_bound(np.abs(proj[0]) @ np.abs(recorded["normalizer"][0]), xc, 3).reshape(ref.shape)
    assert (np.abs(cut - ref) <= bound).all()
    assert full.shape == (2, s, k)


def test_modules_refuse_what_the_kernels_do_not_take():
    sfa = DR.SFALinear(4).to(DEV)
    with pytest.raises(ValueError, match=r"expected \[N, S, 4\]"):
        sfa.update(torch.zeros(5, 4, device=DEV))
    with pytest.raises(ValueError, match="at least 2 are required"):
        sfa.update(torch.zeros(5, 1, 4, device=DEV))
    with pytest.raises(TypeError, match="fp32 only"):
        sfa.update(torch.zeros(5, 3, 4, device=DEV, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no update has run"):
        sfa.build()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sfa.update(torch.zeros(5, 3, 4))
    sfa.update(torch.zeros(5, 2, 4, device=DEV))                          # one kept frame per window: no difference
    with pytest.raises(ValueError, match="no frame-to-frame difference"):
        sfa.build()


# --------------------------------------------------------------------------- the tools, end to end
def test_tools_end_to_end_into_abx(tmp_path):
    """Fit SFA with the tool on the nine files of test_db, export behind it, score with eval_ABX from_pre_computed; a second fit
    with --exact_counts has S / (S - 1) times the mean."""
    window, frames = 5120, 32
    base = [CKPT, None, "--pathDB", DB, "--recursionLevel", "2", "--extension", ".flac", "--sizeWindow", str(window)]
    fits = {}
    for name, flags in (("sfa", []), ("exact", ["--exact_counts"])):
        argv = list(base) + flags
        argv[1] = str(tmp_path / f"{name}.pt")
        fits[name] = DR.main(argv)
        saved = torch.load(tmp_path / f"{name}.pt")
        assert set(saved) == {"state_dict", "inDim", "type"} and saved["type"] == "SFA" and saved["inDim"] == 32
        assert tuple(saved["state_dict"]) == SFA_BUFFERS
        written = json.load(open(tmp_path / f"{name}_args.json"))
        assert written["mode"] == "SFA" and written["sizeWindow"] == window and written["exact_counts"] == bool(flags)
    sfa, exact = fits["sfa"], fits["exact"]
    assert sfa.N_x > 0 and sfa.N_x % frames == 0 and sfa.rows_summed == sfa.N_x // frames * (frames - 1)
    assert np.allclose(exact.solution["mean_x"], sfa.solution["mean_x"] * frames / (frames - 1), rtol=8 * DO.U53, atol=0)
    assert (np.diff(sfa.PCA_values.cpu().numpy()) >= 0).all()
    with pytest.raises(SystemExit, match="exists"):
        DR.main(list(base[:1]) + [str(tmp_path / "sfa.pt")] + base[2:])   # an existing output is not overwritten

    out = tmp_path / "features"
    BR.main([DB, str(out), CKPT, str(tmp_path / "sfa.pt"), "--format", "pt", "--file_extension", ".flac"])
    files = sorted(p.name for p in out.iterdir())
    assert len(files) == 10 and "reduced_args.json" in files
    for name in files:
        if name.endswith(".pt"):
            feat = torch.load(out / name)
            assert feat.dtype == torch.float32 and not feat.is_cuda and feat.dim() == 2 and feat.size(1) == 32
            assert torch.isfinite(feat).all()
    random.seed(2024)
    scores = eval_ABX.main(["from_pre_computed", os.path.join(GOLDEN, "g19_abx_test_db.item"), str(out), "--out",
                            str(tmp_path / "abx")])
    written = json.load(open(tmp_path / "abx" / "ABX_scores.json"))
    assert set(written) == {"within", "across"} and written == scores
    assert all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in written.values())
    with pytest.raises(ValueError, match="not an empty directory"):
        BR.main([DB, str(out), CKPT, str(tmp_path / "sfa.pt")])
