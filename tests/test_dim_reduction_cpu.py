"""cpc2_amd.dim_reduction without a GPU: the numpy statement of tests/dim_reduction_oracle.py against the reference's recorded fits
(golden g29, tools/make_golden_dim_reduction.py), the reference's counts, the three new C entry points' declarations and refusals,
both command lines and what they refuse before the audio is listed, and loadDimReduction's two refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import dim_reduction_oracle as DO
from cpc2_amd import _lib
from cpc2_amd import dataset as ds
from cpc2_amd import dim_reduction as DR
from cpc2_amd.eval import build_reduced_features as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CKPT = os.path.join(GOLDEN, "ref_checkpoint", "checkpoint_7.pt")
CASES = [("k8", 3, 16, 8), ("k64", 6, 40, 64)]
# the maker holds the statement to 1e-8 of the reference (measured there: below 1e-13 at these sizes, 6.4e-10 at k = 256)
LIMIT = 1e-8
PCA_BUFFERS = ("var", "mean", "PCA_mul", "PCA_values")
SFA_BUFFERS = ("covar_speed", "mean_x", "square_x", "covar_x", "normalizer", "PCA_mul", "PCA_values", "projection")


@pytest.fixture(scope="module")
def g29():
    with np.load(os.path.join(GOLDEN, "g29_dim_reduction.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _deviation(mine, g, prefix, names):
    worst = 0.0
    for name in names:
        a, b = np.asarray(mine[name], np.float64), g[f"{prefix}_{name}"]
        if name in ("PCA_mul", "projection"):
            a, b = DO.sign_rule(a[0]), DO.sign_rule(b[0])
        assert a.shape == b.shape, name
        worst = max(worst, float(np.abs(a - b).max() / np.abs(b).max()))
    return worst


def test_golden_holds_the_two_cases(g29):
    assert [str(t) for t in g29["tags"]] == [c[0] for c in CASES]
    for tag, b, s, k in CASES:
        assert g29[f"{tag}_x"].shape == (b, s, k) and g29[f"{tag}_x"].dtype == np.float32
        assert g29[f"{tag}_held_out"].shape == (2, s, k) and g29[f"{tag}_held_out"].dtype == np.float32
        assert float(g29[f"{tag}_deviation"]) <= LIMIT
        assert DO.relative_gap(g29[f"{tag}_sfa_PCA_values"]) >= 1e-4 and DO.relative_gap(g29[f"{tag}_pca_PCA_values"]) >= 1e-4
        assert (np.diff(g29[f"{tag}_sfa_PCA_values"]) > 0).all() and (np.diff(g29[f"{tag}_pca_PCA_values"]) > 0).all()
        assert np.array_equal(DO.ar1_features(b + 2, s, k, int(g29["seed"]) + [c[0] for c in CASES].index(tag))[:b], g29[f"{tag}_x"])


@pytest.mark.parametrize("tag,b,s,k", CASES)
def test_reference_counts_and_raw_sums(g29, tag, b, s, k):
    """3 windows of 16 frames: N_x = 48 for 45 summed rows, N_speed = 45 for 42 differences.  The recorded raw sums are those of
    frames 1 .. s-1 and of the differences between them, exactly (the inputs lie on a grid of 2^-10)."""
    assert (int(g29[f"{tag}_sfa_N_x"]), int(g29[f"{tag}_sfa_N_speed"])) == DO.counts(b, s, exact=False) == (b * s, b * (s - 1))
    assert DO.counts(b, s, exact=True) == (b * (s - 1), b * (s - 2))
    if tag == "k8":
        assert DO.counts(3, 16, False) == (48, 45) and DO.counts(3, 16, True) == (45, 42)
    assert int(g29[f"{tag}_pca_N"]) == b * s
    sums, gram, dgram = DO.seq_moments(g29[f"{tag}_x"], 1)
    assert np.array_equal(sums, g29[f"{tag}_sfa_raw_mean_x"]) and np.array_equal(gram, g29[f"{tag}_sfa_raw_covar_x"])
    assert np.array_equal(dgram, g29[f"{tag}_sfa_raw_covar_speed"])
    assert np.array_equal(np.diag(gram), g29[f"{tag}_sfa_raw_square_x"])
    sums, gram, _ = DO.seq_moments(g29[f"{tag}_x"], 0)
    assert np.array_equal(sums, g29[f"{tag}_pca_raw_mean"]) and np.array_equal(gram, g29[f"{tag}_pca_raw_var"])
    # on the grid the exact integer statement says the same
    xi = np.round(g29[f"{tag}_x"].astype(np.float64) * 1024.0).astype(np.int64)
    si, gi, di = DO.seq_moments_int(xi, 1)
    assert np.array_equal(si / 1024.0, g29[f"{tag}_sfa_raw_mean_x"]) and np.array_equal(di / 1024.0 ** 2, dgram)


@pytest.mark.parametrize("tag,b,s,k", CASES)
def test_statement_reproduces_the_reference_builds(g29, tag, b, s, k):
    x = g29[f"{tag}_x"]
    sums, gram, _ = DO.seq_moments(x, 0)
    dev = _deviation(DO.pca_build(sums, gram, b * s), g29, f"{tag}_pca", PCA_BUFFERS)
    print(tag, "PCA deviation", dev)
    assert dev <= LIMIT
    sums, gram, dgram = DO.seq_moments(x, 1)
    built = DO.sfa_build(sums, gram, dgram, *DO.counts(b, s, exact=False))
    dev = _deviation(built, g29, f"{tag}_sfa", SFA_BUFFERS)
    print(tag, "SFA deviation", dev)
    assert dev <= LIMIT
    # with the exact counts the mean is s / (s - 1) of the reference's
    exact = DO.sfa_build(sums, gram, dgram, *DO.counts(b, s, exact=True))
    assert np.allclose(exact["mean_x"], built["mean_x"] * s / (s - 1), rtol=4 * DO.U53 * 2, atol=0)


@pytest.mark.parametrize("tag,b,s,k", CASES)
def test_statement_reproduces_the_reference_forwards(g29, tag, b, s, k):
    held = g29[f"{tag}_held_out"]
    pca = {n: g29[f"{tag}_pca_{n}"] for n in PCA_BUFFERS}
    sfa = {n: g29[f"{tag}_sfa_{n}"] for n in SFA_BUFFERS}
    for got, ref in ((DO.pca_forward(pca, held), g29[f"{tag}_pca_forward"]),
                     (DO.sfa_forward(sfa, held), g29[f"{tag}_sfa_forward"]),
                     (DO.sfa_forward(sfa, held, sfa["PCA_mul"][:, g29[f"{tag}_sfa_select"] > 0]), g29[f"{tag}_sfa_forward_selected"])):
        assert got.shape == ref.shape and np.abs(got - ref).max() <= LIMIT * np.abs(ref).max()
    assert g29[f"{tag}_sfa_forward_selected"].shape == (2, s, k // 2)
    # projection . normalizer as one matrix gives the same forward
    folded = sfa["projection"][0] @ sfa["normalizer"][0]
    rows = (held.astype(np.float64).reshape(-1, k) - sfa["mean_x"]) / (sfa["square_x"] + 1e-08)
    assert np.abs((rows @ folded.T).reshape(2, s, k) - g29[f"{tag}_sfa_forward"]).max() <= 1e-11 * np.abs(g29[f"{tag}_sfa_forward"]).max()


def test_modules_keep_the_references_state_dict(g29):
    pca, sfa = DR.PCA(8), DR.SFALinear(8)
    assert tuple(pca.state_dict()) == PCA_BUFFERS and tuple(sfa.state_dict()) == SFA_BUFFERS
    for name in PCA_BUFFERS:
        assert tuple(pca.state_dict()[name].shape) == g29[f"k8_pca_{name}"].shape
    for name in SFA_BUFFERS:
        assert tuple(sfa.state_dict()[name].shape) == g29[f"k8_sfa_{name}"].shape
    assert pca.building and sfa.building and (pca.N, sfa.N_x, sfa.N_speed) == (0, 0, 0) and not sfa.exact_counts
    assert DR.SFALinear(8, exact_counts=True).exact_counts
    for bad in (0, 513):
        with pytest.raises(ValueError, match="outside the supported limits"):
            DR.PCA(bad)
        with pytest.raises(ValueError, match="outside the supported limits"):
            DR.SFALinear(bad)
    # no CPU fallback, for update and for forward
    for module in (pca, sfa):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            module.update(torch.zeros(2, 5, 8))
        module.building = False
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            module(torch.zeros(2, 5, 8))


def _reference_file(g, tag, kind, path, **extra):
    names = PCA_BUFFERS if kind == "PCA" else SFA_BUFFERS
    state = {n: torch.from_numpy(g[f"{tag}_{kind.lower()}_{n}"]).float() for n in names}
    torch.save(dict({"state_dict": state, "inDim": int(g[f"{tag}_x"].shape[2]), "type": kind}, **extra), path)


def test_load_dim_reduction_and_its_refusals(g29, tmp_path):
    _reference_file(g29, "k8", "SFA", tmp_path / "sfa.pt")
    _reference_file(g29, "k8", "PCA", tmp_path / "pca.pt")
    sfa = DR.loadDimReduction(str(tmp_path / "sfa.pt"), None)
    assert isinstance(sfa, DR.SFALinear) and not sfa.building and sfa.k == 8
    assert np.array_equal(sfa.normalizer.numpy(), g29["k8_sfa_normalizer"].astype(np.float32))
    pca = DR.loadDimReduction(str(tmp_path / "pca.pt"), None)
    assert isinstance(pca, DR.PCA) and not pca.building
    with pytest.raises(ValueError, match="no 'centroid_values'"):
        DR.loadDimReduction(str(tmp_path / "sfa.pt"), [0, 1])
    with pytest.raises(ValueError, match="holds a PCA.*centroidLimits"):
        DR.loadDimReduction(str(tmp_path / "pca.pt"), [0, 1])
    torch.save({"state_dict": {}, "inDim": 8, "type": "ICA"}, tmp_path / "ica.pt")
    with pytest.raises(ValueError, match="Invalid module type ICA"):
        DR.loadDimReduction(str(tmp_path / "ica.pt"), None)
    # with centroid_values the limits select rows of PCA_mul, strictly between the two
    _reference_file(g29, "k8", "SFA", tmp_path / "sfa_c.pt", centroid_values=torch.arange(8.0))
    cut = DR.loadDimReduction(str(tmp_path / "sfa_c.pt"), [1, 5])
    assert tuple(cut.projection.shape) == (1, 3, 8) and torch.equal(cut.projection[0], cut.PCA_mul[0, 2:5])
    assert DR.ModelDimReduced(torch.nn.Identity(), cut).out_feature_dim == 3
    assert DR.ModelDimReduced(torch.nn.Identity(), pca).out_feature_dim == 8
    # save writes the reference's three keys, and a projection cut by selectDimensions loads back
    cut.save(str(tmp_path / "cut.pt"))
    saved = torch.load(tmp_path / "cut.pt")
    assert set(saved) == {"state_dict", "inDim", "type"} and saved["type"] == "SFA" and saved["inDim"] == 8
    assert tuple(saved["state_dict"]) == SFA_BUFFERS
    back = DR.loadDimReduction(str(tmp_path / "cut.pt"), None)
    assert torch.equal(back.projection, cut.projection)


# --------------------------------------------------------------------------- the command lines
def test_fit_tool_parses_the_references_flags():
    args = DR.parseArgs(["c.pt", "o.pt", "--pathDB", "db"])
    assert vars(args) == dict(pathCheckpoint="c.pt", pathOut="o.pt", pathDB="db", seqList=None, recursionLevel=2, extension=".flac",
                              mode="SFA", debug=False, batchSize=8, sizeWindow=20480, exact_counts=False)
    args = DR.parseArgs(["c.pt", "o.pt", "--pathDB", "db", "--seqList", "l.txt", "--recursionLevel", "1", "--extension", ".wav",
                         "--mode", "PCA", "--debug", "--batchSize", "4", "--sizeWindow", "10240", "--exact_counts"])
    assert (args.seqList, args.recursionLevel, args.extension, args.mode, args.debug, args.batchSize, args.sizeWindow,
            args.exact_counts) == ("l.txt", 1, ".wav", "PCA", True, 4, 10240, True)
    with pytest.raises(SystemExit):
        DR.parseArgs(["c.pt", "o.pt"])                                   # --pathDB is required
    with pytest.raises(SystemExit):
        DR.parseArgs(["c.pt", "o.pt", "--pathDB", "db", "--mode", "ICA"])


def test_export_tool_parses_its_flags():
    args = BR.parse_args(["a", "o", "c.pt", "d.pt"])
    assert vars(args) == dict(path_audio="a", path_out="o", pathCheckpoint="c.pt", pathDimReduction="d.pt", centroidLimits=None,
                              format="pt", file_extension=".flac", maxSizeSeq=64000, strict=False, seqNorm=False)
    args = BR.parse_args(["a", "o", "c.pt", "d.pt", "--centroidLimits", "1", "5", "--format", "fea", "--file_extension", ".wav",
                          "--maxSizeSeq", "32000", "--strict", "--seqNorm"])
    assert (args.centroidLimits, args.format, args.file_extension, args.maxSizeSeq, args.strict, args.seqNorm) == \
        ([1.0, 5.0], "fea", ".wav", 32000, True, True)


def test_fit_tool_refuses_by_name_before_the_audio_is_listed(monkeypatch, tmp_path):
    listed = []
    monkeypatch.setattr(ds, "findAllSeqs", lambda *a, **k: listed.append(a) or ([], []))
    out = tmp_path / "out.pt"
    exists = tmp_path / "exists.pt"
    exists.write_bytes(b"")
    for argv, text in [([CKPT, str(out), "--pathDB", "db", "--extension", ".mp3"], r"--extension \.mp3: there is no mp3 decoder"),
                       (["missing/checkpoint_1.pt", str(out), "--pathDB", "db"], "pathCheckpoint missing/checkpoint_1.pt: not an existing"),
                       ([os.path.join(GOLDEN, "ref_checkpoint", "checkpoint_args.json"), str(out), "--pathDB", "db"],
                        "pathCheckpoint .*not an existing .pt"),
                       ([CKPT, str(exists), "--pathDB", "db"], "pathOut .*exists.pt exists"),
                       ([CKPT, str(out), "--pathDB", "db", "--batchSize", "0"], "--batchSize 0")]:
        with pytest.raises(SystemExit, match=text):
            DR.main(argv)
    assert not listed and not out.exists() and exists.read_bytes() == b""


def test_export_tool_refuses_by_name_before_the_audio_is_listed(g29, monkeypatch, tmp_path):
    listed = []
    monkeypatch.setattr(ds, "findAllSeqs", lambda *a, **k: listed.append(a) or ([], []))
    _reference_file(g29, "k8", "SFA", tmp_path / "sfa.pt")
    _reference_file(g29, "k8", "PCA", tmp_path / "pca.pt")
    full = tmp_path / "full"
    full.mkdir()
    (full / "x.pt").write_bytes(b"")
    out, sfa, pca = str(tmp_path / "out"), str(tmp_path / "sfa.pt"), str(tmp_path / "pca.pt")
    for argv, kind, text in [(["db", str(full), CKPT, sfa], ValueError, "full exists and is not an empty directory"),
                             (["db", out, CKPT, sfa, "--file_extension", ".mp3"], NotImplementedError, r"--file_extension \.mp3"),
                             (["db", out, "missing.pt", sfa], ValueError, "pathCheckpoint missing.pt: not an existing .pt file"),
                             (["db", out, CKPT, "missing.pt"], ValueError, "pathDimReduction missing.pt: not an existing .pt file"),
                             (["db", out, CKPT, sfa, "--centroidLimits", "0", "1"], ValueError, "no 'centroid_values'"),
                             (["db", out, CKPT, pca, "--centroidLimits", "0", "1"], ValueError, "holds a PCA")]:
        with pytest.raises(kind, match=text):
            BR.main(argv)
    assert not listed and not os.path.exists(out) and sorted(p.name for p in full.iterdir()) == ["x.pt"]


# --------------------------------------------------------------------------- the C entry points
NEW_SYMBOLS = ("cpc_seq_moments_scratch_bytes", "cpc_seq_moments_accumulate", "cpc_center_scale_rows")


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "cpc2_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in cpc2_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES
    assert _lib.load().cpc_version() >= 121


def test_seq_moments_refuses_before_any_launch():
    lib = _lib.load()
    query = lib.cpc_seq_moments_scratch_bytes
    assert query(1, 1, 0, 1) > 0 and query(1, 2, 1, 3) > 0 and query(1 << 10, 1 << 20, 1, 512) > 0
    assert query(1, (1 << 31) - 1, 0, 512) > 0
    one = ctypes.c_void_p(256)                                          # never dereferenced: refused before any launch

    def call(b, s, skip, d, ld=None, seq_stride=None, x=one, sums=one, gram=one, dgram=one, scratch=one, nbytes=1 << 40):
        ld = d if ld is None else ld
        return lib.cpc_seq_moments_accumulate(x, ld, s * ld if seq_stride is None else seq_stride, b, s, skip, d, sums, gram, dgram,
                                              scratch, nbytes, None)
    for b, s, skip, d in [(0, 4, 1, 4), (-1, 4, 1, 4), (2, 4, 1, 0), (2, 4, 1, 513), (2, 4, 4, 4), (2, 4, -1, 4), (2, 0, 0, 4),
                          (2, 1, 1, 4), (1 << 11, 1 << 20, 1, 4)]:
        assert query(b, s, skip, d) == 0, (b, s, skip, d)
        assert call(b, s, skip, d) == -1 and b"sizes outside the supported limits" in lib.cpc_last_error(), (b, s, skip, d)
    assert call(2, 4, 1, 4, ld=3) == -1 and b"stride below the width" in lib.cpc_last_error()
    assert call(2, 4, 1, 4, ld=5, seq_stride=19) == -1 and b"stride below the width" in lib.cpc_last_error()
    for missing in ("x", "sums", "gram", "dgram"):
        assert call(2, 4, 1, 4, **{missing: None}) == -1 and b"null buffer" in lib.cpc_last_error(), missing
    assert call(2, 4, 1, 4, scratch=None) == -1 and b"scratch" in lib.cpc_last_error()
    assert call(2, 4, 1, 4, nbytes=16) == -1 and b"scratch" in lib.cpc_last_error()


def test_center_scale_rows_refuses_before_any_launch():
    lib = _lib.load()
    one, two = ctypes.c_void_p(256), ctypes.c_void_p(1 << 20)

    def call(n, d, ldx=None, ldy=None, x=one, mean=one, scale=one, y=two):
        return lib.cpc_center_scale_rows(x, d if ldx is None else ldx, mean, scale, y, d if ldy is None else ldy, n, d, None)
    for n, d in [(0, 4), (-3, 4), (5, 0), (5, 513), (5, -1)]:
        assert call(n, d) == -1 and b"sizes outside the supported limits" in lib.cpc_last_error(), (n, d)
    assert call(5, 4, ldx=3) == -1 and b"row stride" in lib.cpc_last_error()
    assert call(5, 4, ldy=3) == -1 and b"row stride" in lib.cpc_last_error()
    for missing in ("x", "mean", "y"):
        assert call(5, 4, **{missing: None}) == -1 and b"null buffer" in lib.cpc_last_error(), missing
    assert call(5, 4, ldx=6, ldy=4, y=one) == -1 and b"in place needs ldy == ldx" in lib.cpc_last_error()
