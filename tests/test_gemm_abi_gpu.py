"""cpc_gemm_nt / cpc_gemm_tn off the training shapes: free leading dimensions, misaligned bases, padded outputs, every kernel
and epilogue the launchers (cpc2_amd/csrc/gemm_f32.hip: gemm_nt, gemm_tn) can pick, and the top of the f32 range.

Harness.  Every operand is a window of a larger buffer that the test owns and has filled with NaN: `front` floats before the
window (front % 4 gives the misalignment of the base), the padding of each row up to its leading dimension, and one more row
of NaN behind it.  The output buffer holds ONE NaN bit pattern; afterwards it is compared as int32, so a store outside the
M x N window -- one column past N, the padding up to ldc, before the base, behind the last row -- changes a word that must not
change, and a read of padding that reaches an output shows as a NaN inside the window.  Nothing relies on a fault.

Reference: the fp64 product of the same f32 values.  Bounds, both the project's own (tests/test_gpu_parity.py):
  * assert_close(c, ref, 2e-6 * max(1, K ** 0.5))                                    (test_gemm_nt / test_gemm_tn)
  * element by element |C - C64| <= 16 * 2^-24 * (|A| . |B| + |bias|)                (test_gemm_split_accuracy, K <= 2048)
Every case keeps the reduction length <= 2048, where both bounds are already held; the one longer TN product, R = 4000, is
added up by the launcher in 32 slabs of 128 rows.

The unmarked tests at the end need no GPU: they hold the case list to a mirror of the launchers' predicates (so that a case
stays on the kernel it names) and run the buffer builder and the checker against a plain torch implementation and against
three deliberately wrong ones, which must be rejected.
"""
import collections
import functools
import math

import pytest
import torch

from cpc2_amd import _lib

DEV = "cuda:0"
NAN_WORD = 0x7FC0BEEF              # the one bit pattern of the output buffer: a quiet NaN no arithmetic produces
FRONT = 8                          # floats of poison before every window (+ the misalignment of the case)
U = 2.0 ** -24


def _cdiv(a, b):
    return -(-a // b)


# ----------------------------------------------------------------------------------------------------------------- the cases
# kind "nt": C[m,n] = A[m,k] . B[n,k]^T (+ bias);  kind "tn": C[m,n] = sum_r A[r,m] B[r,n], k = the row count R.
# lda / ldb / ldc None: dense.  a_off / b_off / c_off: floats by which the base is off a 16-byte boundary.
# expect: what the launcher does with the case (checked against the mirror below by test_cases_reach_the_kernels_they_name).
Case = collections.namedtuple("Case", "kind m n k lda ldb ldc a_off b_off c_off bias mode expect")


def _case(kind, m, n, k, expect, lda=None, ldb=None, ldc=None, a_off=0, b_off=0, c_off=0, bias=False, mode=0):
    dense_a, dense_b = (k, k) if kind == "nt" else (m, n)
    return Case(kind, m, n, k, lda or dense_a, ldb or dense_b, ldc or n, a_off, b_off, c_off, bias, mode, expect)


def _id(c):
    dense = _case(c.kind, c.m, c.n, c.k, None)
    extra = [f"{f}{getattr(c, f)}" for f in ("lda", "ldb", "ldc", "a_off", "b_off", "c_off") if getattr(c, f) != getattr(dense, f)]
    return "-".join([c.kind, f"{c.m}x{c.n}x{c.k}"] + extra + (["bias"] if c.bias else []) + ([f"mode{c.mode}"] if c.mode else []))


UNALIGNED_NT, F32_NT_64, F32_NT_128 = "gemm_nt_kernel<false,2>", "gemm_nt_kernel<true,1>", "gemm_nt_kernel<true,2>"
X6_64, X6_128x256 = "gemm_nt_x6_kernel<1,2>", "gemm_nt_x6_kernel<2,4>"
UNALIGNED_TN, F32_TN, X6P_TN = "gemm_tn_kernel<false>", "gemm_tn_kernel<true>", "gemm_tn_x6p_kernel"

NT_CASES = [
    # a.aligned is false (K % 4 != 0): gemm_nt_kernel<false,2>, 2 x 2 tiles of 128 x 128, K = 2 * 32 + 13
    _case("nt", 193, 130, 77, dict(kernel=UNALIGNED_NT, blocks=4, splits=1, ktail=True), bias=True),
    # a.aligned is false through lda % 4 / ldb % 4 alone (K % 4 == 0, bases aligned)
    _case("nt", 150, 140, 64, dict(kernel=UNALIGNED_NT, blocks=4, ktail=False), lda=65, ldb=67),
    # ... and through the base of A, of B alone
    _case("nt", 150, 140, 64, dict(kernel=UNALIGNED_NT, blocks=4), a_off=1, bias=True),
    _case("nt", 150, 140, 64, dict(kernel=UNALIGNED_NT, blocks=4), b_off=3),
    # aligned, 3 * 2 tiles of 128 < 512 -> 64-row tiles; ldc != N: no split; N, ldc % 4 == 0, C aligned -> vec_out (staged
    # 16-byte stores) with a row stride above N
    _case("nt", 300, 200, 72, dict(kernel=X6_64, blocks=10, splits=1, epilogue="staged", xcd=False, ktail=True), ldc=208, bias=True),
    # vec_out off because ldc % 4 != 0, because C % 16 != 0
    _case("nt", 300, 200, 72, dict(kernel=X6_64, epilogue="scalar"), ldc=203),
    _case("nt", 300, 200, 72, dict(kernel=X6_64, epilogue="scalar"), c_off=1, bias=True),
    # all three leading dimensions above the extents, still aligned
    _case("nt", 300, 200, 72, dict(kernel=X6_64, epilogue="staged", ktail=True), lda=80, ldb=76, ldc=208),
    # one tile, K = 2048, ldc == N: nt_splits -> 4 parts of 512, C zeroed, atomics, bias from blockIdx.y == 0 only
    _case("nt", 64, 128, 2048, dict(kernel=X6_64, blocks=1, splits=4, epilogue="atomic"), bias=True),
    # the same product with ldc != N: the split is suppressed (the memset covers a dense C only)
    _case("nt", 64, 128, 2048, dict(kernel=X6_64, blocks=1, splits=1, epilogue="staged"), ldc=132, bias=True),
    # N == 256 and 512 row tiles of 128 fill the chip twice: 128 x 256 tile; last row tile holds 78 rows; one panel: no remap
    _case("nt", 65486, 256, 32, dict(kernel=X6_128x256, blocks=512, xcd=False, epilogue="staged")),
    # 256 row tiles (% 8 == 0) x 2 panels of 256: 128 x 256 tile with xcd_remap; last row tile holds 60 rows
    _case("nt", 32700, 512, 32, dict(kernel=X6_128x256, blocks=512, xcd=True), bias=True),
    # 64-row tiles, 8 resp. 24 of them (% 8 == 0), 2 resp. 3 panels: xcd_remap; K = 64 (no tail), K = 40 (tail)
    _case("nt", 512, 256, 64, dict(kernel=X6_64, blocks=16, xcd=True, ktail=False)),
    _case("nt", 1536, 384, 40, dict(kernel=X6_64, blocks=72, xcd=True, ktail=True), bias=True),
    # smallest aligned K: N % 4 == 0 -> staged, N % 4 != 0 -> scalar
    _case("nt", 2, 4, 4, dict(kernel=X6_64, blocks=1, epilogue="staged"), bias=True),
    _case("nt", 5, 3, 4, dict(kernel=X6_64, blocks=1, epilogue="scalar")),
    # mode 1: the f32-MFMA kernels at ragged M, N and a K tail; < 512 tiles of 128 -> <true,1>, 547 * 2 tiles -> <true,2>
    _case("nt", 300, 200, 72, dict(kernel=F32_NT_64, blocks=10, ktail=True), bias=True, mode=1),
    _case("nt", 1100, 130, 100, dict(kernel=F32_NT_64, blocks=36, ktail=True), mode=1),
    _case("nt", 70000, 130, 36, dict(kernel=F32_NT_128, blocks=1094, ktail=True), bias=True, mode=1),
]

TN_CASES = [
    # M % 4 != 0: gemm_tn_kernel<false>; 2 x 3 tiles, 8 row slabs of 128 (the last holds 104); N % 4 != 0: scalar reduce, S = 8
    _case("tn", 130, 258, 1000, dict(kernel=UNALIGNED_TN, tiles=6, slabs=8, reduce="scalar")),
    # odd N: the scalar slab stores; the second column tile is one column wide
    _case("tn", 96, 129, 333, dict(kernel=UNALIGNED_TN, tiles=2, slabs=3, reduce="scalar")),
    # ... written through ldc > N into a misaligned C
    _case("tn", 96, 129, 333, dict(kernel=UNALIGNED_TN, tiles=2, slabs=3), ldc=131, c_off=3),
    # smallest extents: two slabs (128 + 72 rows); one row, one element
    _case("tn", 5, 3, 200, dict(kernel=UNALIGNED_TN, tiles=1, slabs=2)),
    _case("tn", 1, 1, 1, dict(kernel=UNALIGNED_TN, tiles=1, slabs=1)),
    # aligned with every leading dimension above its extent: the pipelined split kernel; 4 slabs, the last 116 rows (7 stages + 4)
    _case("tn", 128, 256, 500, dict(kernel=X6P_TN, tiles=2, slabs=4, xcd=False, reduce="float4"), lda=132, ldb=260, ldc=264),
    # a.aligned false through lda % 4, the base of A, the base of B (M, N % 4 == 0)
    _case("tn", 128, 256, 500, dict(kernel=UNALIGNED_TN, slabs=4), lda=129),
    _case("tn", 128, 256, 500, dict(kernel=UNALIGNED_TN, slabs=4), a_off=1),
    _case("tn", 128, 256, 500, dict(kernel=UNALIGNED_TN, slabs=4), b_off=2),
    # S % 8 == 0 and several tiles: xcd_remap, with S = 8 and S = 32 (N = 4: every column pair clamped to N - 2)
    _case("tn", 256, 128, 1024, dict(kernel=X6P_TN, tiles=2, slabs=8, xcd=True)),
    _case("tn", 300, 4, 4000, dict(kernel=X6P_TN, tiles=3, slabs=32, xcd=True)),
    # row ranges shorter than two / one 16-row stage of the pipeline (its prologue loads stages 0, 1, 2 whatever nk is)
    _case("tn", 132, 260, 17, dict(kernel=X6P_TN, tiles=6, slabs=1)),
    _case("tn", 4, 4, 1, dict(kernel=X6P_TN, tiles=1, slabs=1)),
    _case("tn", 8, 12, 15, dict(kernel=X6P_TN, tiles=1, slabs=1)),
    # mode 1: unaligned stays on gemm_tn_kernel<false>; aligned takes gemm_tn_kernel<true> (ragged M, N: clamped 16-byte loads)
    _case("tn", 130, 258, 1000, dict(kernel=UNALIGNED_TN, slabs=8), mode=1),
    _case("tn", 132, 260, 1000, dict(kernel=F32_TN, tiles=6, slabs=8), mode=1),
]


# ------------------------------------------------------------------------------------------------- mirror of the launchers
def nt_dispatch(c):
    """gemm_nt's choices for a call without a row map (the C entry), from the same predicates in the same order."""
    m, n, k = c.m, c.n, c.k
    aligned = k % 4 == 0 and k >= 4 and c.lda % 4 == 0 and c.ldb % 4 == 0 and c.a_off % 4 == 0 and c.b_off % 4 == 0
    native = c.mode == 1
    split_kernels = aligned and not native
    mi, nj = 2, 2
    if split_kernels and n % 256 == 0 and _cdiv(m, 128) * (n // 256) >= 512:
        def fill(blocks, places):
            return blocks / (_cdiv(blocks, places) * places)
        wide, narrow = 165.0 * fill(_cdiv(m, 128) * (n // 256), 512), 150.0 * fill(_cdiv(m, 128) * (n // 128), 768)
        nj = 4 if (n == 256 or wide >= narrow) else 2
    elif aligned and _cdiv(m, 128) * _cdiv(n, 128) < 512:
        mi = 1
    blocks = _cdiv(m, 64 * mi) * _cdiv(n, 64 * nj)
    splits = 1
    if aligned and c.ldc == n and not (blocks >= 512 or k < 2048):
        splits = max(1, min(_cdiv(768, blocks), k // 512))
    kchunk = _cdiv(_cdiv(k, splits), 32) * 32
    splits = _cdiv(k, kchunk)
    xcd = split_kernels and _cdiv(n, 64 * nj) > 1 and _cdiv(m, 64 * mi) % 8 == 0
    vec_out = splits == 1 and n % 4 == 0 and c.ldc % 4 == 0 and c.c_off % 4 == 0
    if not aligned:
        kernel = UNALIGNED_NT
    elif native:
        kernel = F32_NT_64 if mi == 1 else F32_NT_128
    else:
        kernel = X6_128x256 if nj == 4 else X6_64 if mi == 1 else "gemm_nt_x6_kernel<2,2>"
    epilogue = "atomic" if splits > 1 else "staged" if (vec_out and split_kernels) else "scalar"
    return dict(kernel=kernel, blocks=blocks, splits=splits, xcd=bool(xcd), epilogue=epilogue, ktail=k % 32 != 0)


def tn_slabs(m, n, r):
    tiles = _cdiv(m, 128) * _cdiv(n, 128)
    s = max(1, min(768 // tiles, _cdiv(r, 128)))
    chunk = _cdiv(_cdiv(r, s), 32) * 32
    return _cdiv(r, chunk)


def tn_dispatch(c):
    m, n, r = c.m, c.n, c.k
    aligned = (m % 4 == 0 and n % 4 == 0 and m >= 4 and n >= 4 and c.lda % 4 == 0 and c.ldb % 4 == 0
               and c.a_off % 4 == 0 and c.b_off % 4 == 0)
    tiles, slabs = _cdiv(m, 128) * _cdiv(n, 128), tn_slabs(m, n, r)
    kernel = X6P_TN if (aligned and c.mode != 1) else F32_TN if aligned else UNALIGNED_TN
    return dict(kernel=kernel, tiles=tiles, slabs=slabs, xcd=kernel == X6P_TN and slabs % 8 == 0 and tiles > 1,
                reduce="float4" if n % 4 == 0 else "scalar")


# ------------------------------------------------------------------------------------------------------ values and references
Values = collections.namedtuple("Values", "a b bias ref mag")


def _reference(kind, a, b, bias):
    a64, b64 = a.double(), b.double()
    if kind == "nt":
        ref, mag = a64 @ b64.t(), a64.abs() @ b64.abs().t()
    else:
        ref, mag = a64.t() @ b64, a64.abs().t() @ b64.abs()
    if bias is not None:
        ref, mag = ref + bias.double(), mag + bias.double().abs()
    return ref, mag


@functools.lru_cache(maxsize=2)
def _values(kind, m, n, k, with_bias):
    """f32 operands of a shape and the fp64 product of those same values; shared by the cases of one shape."""
    g = torch.Generator().manual_seed(1000003 * m + 1009 * n + k + (7 if kind == "tn" else 0))
    if kind == "nt":
        a, b = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g)
    else:
        a, b = torch.randn(k, m, generator=g), torch.randn(k, n, generator=g)
    bias = torch.randn(n, generator=g) if with_bias else None
    return Values(a, b, bias, *_reference(kind, a, b, bias))


def values_of(c):
    return _values(c.kind, c.m, c.n, c.k, c.bias)


# ------------------------------------------------------------------------------------------------------------------ buffers
class Operands:
    """The three poisoned buffers of a call.  x_buf is the flat allocation, x_at the element offset of the window's base."""

    def __init__(self, c, vals, device):
        self.a_buf, self.a_at, self.a = _operand(vals.a, c.lda, c.a_off, device)
        self.b_buf, self.b_at, self.b = _operand(vals.b, c.ldb, c.b_off, device)
        self.c_at = FRONT + c.c_off
        self.c_words = torch.full((self.c_at + (c.m - 1) * c.ldc + c.n + c.ldc + 5,), NAN_WORD, dtype=torch.int32, device=device)
        self.c_buf = self.c_words.view(torch.float32)
        self.c = self.c_buf.as_strided((c.m, c.n), (c.ldc, 1), self.c_at)
        self.bias = vals.bias.to(device) if vals.bias is not None else None
        for view, off, name in ((self.a, c.a_off, "A"), (self.b, c.b_off, "B"), (self.c, c.c_off, "C")):
            assert view.data_ptr() % 16 == (4 * off) % 16, f"{name}: base {view.data_ptr():#x} is not {4 * off % 16} bytes off 16"


def _operand(values, ld, off, device):
    rows, cols = values.shape
    assert ld >= cols
    at = FRONT + off
    buf = torch.full((at + (rows - 1) * ld + cols + ld + 5,), float("nan"), dtype=torch.float32, device=device)
    view = buf.as_strided((rows, cols), (ld, 1), at)
    view.copy_(values)
    return buf, at, view


# ------------------------------------------------------------------------------------------------------------------ checker
def assert_close(got, ref, tol, what="", rtol=None):
    """tests/test_gpu_parity.py's check, restated: |got - ref|_inf <= tol * |ref|_inf AND, element by element,
    |got - ref| <= atol + rtol * |ref| with atol = tol * |ref|_inf and rtol = 64 * tol."""
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    e = float((g - r).abs().max() / (r.abs().max() + 1e-30))
    assert e <= tol, f"{what}: rel err {e:.3e} > {tol:.1e}"
    atol = tol * float(r.abs().max()) + 1e-30
    rt = 64 * tol if rtol is None else rtol
    bad = (g - r).abs() > atol + rt * r.abs()
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements outside atol {atol:.2e} + {rt:.1e} |ref|"


def check_output(c, ops, ref, mag, poisoned_rows=(), allowance=None):
    """Every word outside the M x N window still holds NAN_WORD; inside, every value is finite and within both bounds of the
    fp64 product -- except the rows in `poisoned_rows`, which must be non-finite throughout.  `allowance` (test of the bottom
    of the range only): an absolute error per element on top of the second bound, in place of the first."""
    what = _id(c)
    words = ops.c_words.cpu()
    inside = torch.zeros(words.numel(), dtype=torch.bool)
    inside.as_strided((c.m, c.n), (c.ldc, 1), ops.c_at).fill_(True)
    stray = (words != NAN_WORD) & ~inside
    assert not bool(stray.any()), (f"{what}: {int(stray.sum())} words outside the {c.m} x {c.n} window were written, the first at "
                                   f"element {int(stray.nonzero()[0]) - ops.c_at} from the base (ldc {c.ldc})")
    got = words.view(torch.float32).as_strided((c.m, c.n), (c.ldc, 1), ops.c_at)
    keep = torch.ones(c.m, dtype=torch.bool)
    for row in poisoned_rows:
        keep[row] = False
        assert not bool(torch.isfinite(got[row]).any()), f"{what}: row {row} is fed by an element outside the domain but has finite outputs"
    got, ref, mag = got[keep], ref[keep], mag[keep]
    finite = torch.isfinite(got)
    assert bool(finite.all()), f"{what}: {int((~finite).sum())} non-finite outputs inside the window"
    err = (got.double() - ref).abs()
    if allowance is None:
        assert_close(got, ref, 2e-6 * max(1.0, c.k ** 0.5), what)
        over = err > 16 * U * mag
    else:
        over = err > 16 * U * mag + allowance[keep]
    assert not bool(over.any()), (f"{what}: {int(over.sum())} elements beyond 16 * 2^-24 * (|A|.|B| + |bias|), worst "
                                  f"{float((err / mag.clamp_min(1e-300)).max()) / U:.1f} * 2^-24")
    return float((err / mag.clamp_min(1e-300)).max()) / U


# ---------------------------------------------------------------------------------------------------------- the library call
def run_library(c, ops, scratch_bytes=None):
    """The call under test, in GEMM mode c.mode (restored afterwards); returns the status of the entry point."""
    lib = _lib.load()
    st = _lib.stream_ptr(ops.c.device)
    prev = lib.cpc_gemm_set_mode(c.mode)
    try:
        if c.kind == "nt":
            return lib.cpc_gemm_nt(_lib.ptr(ops.a), c.lda, _lib.ptr(ops.b), c.ldb, _lib.ptr(ops.c), c.ldc, _lib.ptr(ops.bias),
                                   c.m, c.n, c.k, st)
        query = lib.cpc_gemm_tn_scratch_bytes(c.m, c.n, c.k)
        nbytes = query if scratch_bytes is None else scratch_bytes
        scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=ops.c.device)
        return lib.cpc_gemm_tn(_lib.ptr(ops.a), c.lda, _lib.ptr(ops.b), c.ldb, _lib.ptr(ops.c), c.ldc, c.m, c.n, c.k,
                               _lib.ptr(scratch), nbytes, st)
    finally:
        lib.cpc_gemm_set_mode(prev)


@pytest.mark.gpu
@pytest.mark.parametrize("case", NT_CASES + TN_CASES, ids=_id)
def test_gemm_entry_points_off_the_training_shapes(case):
    vals = values_of(case)
    ops = Operands(case, vals, DEV)
    _lib.check(run_library(case, ops), _id(case))
    check_output(case, ops, vals.ref, vals.mag)


# the query rounds S * M * N * 4 up to 256 bytes.  (128, 256, 500): 4 slabs, 524288 bytes, already a multiple -- one byte below
# the query is one byte too few; (5, 3, 200): 2 slabs, 120 bytes of a 256-byte query -- one byte below what the slabs take
@pytest.mark.gpu
@pytest.mark.parametrize("m,n,r,below", [(128, 256, 500, "query"), (5, 3, 200, "slabs")])
def test_gemm_tn_refuses_a_scratch_that_is_too_small(m, n, r, below):
    lib = _lib.load()
    case = _case("tn", m, n, r, None)
    query = lib.cpc_gemm_tn_scratch_bytes(m, n, r)
    slabs = tn_slabs(m, n, r) * m * n * 4
    assert query == _cdiv(slabs, 256) * 256
    assert below == "slabs" or query == slabs
    ops = Operands(case, values_of(case), DEV)
    status = run_library(case, ops, scratch_bytes=(query if below == "query" else slabs) - 1)
    assert status == -3, status                                  # CPC_ERR_WORKSPACE
    assert "scratch too small" in lib.cpc_last_error().decode()
    torch.cuda.synchronize()
    assert bool((ops.c_words.cpu() == NAN_WORD).all()), "a refused call wrote to C"


# ------------------------------------------------------------------------------------ the two ends of the f32 range in mode 0
# A split kernel holds every operand as three bf16 terms (split2 in gemm_f32.hip), and bf16 ends before f32 does at both ends:
#   * the largest finite bf16 is (2 - 2^-7) 2^127 = 3.3895e38; round-to-nearest-even takes everything from (2 - 2^-8) 2^127 =
#     3.3962e38 up to +inf, the residual x - inf is -inf and the next one NaN.  Below that the three terms are exact;
#   * the smallest bf16 subnormal is 2^-133 (f32: 2^-149), so the three terms give x to within 2^-134 ABSOLUTE: exact (to
#     2^-27 |x|, as everywhere) from |x| = 2^-110 up, and for the multiples of 2^-133 below that.
BF16_OVERFLOW = (2.0 - 2.0 ** -8) * 2.0 ** 127
BF16_GRID = 2.0 ** -133
TOP_CASES = [_case("nt", 70, 136, 64, dict(kernel=X6_64)), _case("tn", 72, 136, 100, dict(kernel=X6P_TN))]
ROW, KK = 37, 21


def _top_of_range_values(c, big, on_grid):
    """The values of `c` with element (ROW, KK) of the product's left operand set to `big` and everything it is multiplied
    with at 0.9e-38 .. 1.9e-38, so that the f32 product itself stays finite.  on_grid: those partners are multiples of 2^-133
    (100 .. 199 of them), which have an exact split; else they carry every bit f32 has there (a grid of 2^-149)."""
    v = values_of(c)
    a, b = v.a.clone(), v.b.clone()
    g = torch.Generator().manual_seed(5)
    steps = torch.randint(100, 200, (c.n,), generator=g).double()
    if not on_grid:
        steps = steps + torch.rand(c.n, generator=g).double()
    tiny = (steps * BF16_GRID).float()
    assert float(tiny.min()) > 0.9e-38 and float(tiny.max()) < 1.9e-38
    if c.kind == "nt":
        a[ROW, KK] = big
        b[:, KK] = tiny * torch.sign(b[:, KK])
    else:
        a[KK, ROW] = big
        b[KK, :] = tiny * torch.sign(b[KK, :])
    return Values(a, b, None, *_reference(c.kind, a, b, None))


@pytest.mark.gpu
@pytest.mark.parametrize("case", TOP_CASES, ids=_id)
def test_gemm_split_is_exact_up_to_the_largest_bf16(case):
    """An element of 3.0e38 is below the bf16 overflow threshold and splits exactly: against partners of ~1e-38 mode 0 meets
    the same two bounds as everywhere else.  The partners are multiples of 2^-133: at 1e-38 nothing else has an exact split
    (next test; with partners of all f32 bits the NT case is off by 4.05e-4 of |C|_inf against the 1.6e-5 of the first bound)."""
    vals = _top_of_range_values(case, 3.0e38, on_grid=True)
    ops = Operands(case, vals, DEV)
    _lib.check(run_library(case, ops), _id(case))
    check_output(case, ops, vals.ref, vals.mag)


@pytest.mark.gpu
@pytest.mark.parametrize("case", TOP_CASES, ids=_id)
def test_gemm_split_holds_tiny_operands_to_the_bf16_grid(case):
    """The same product with partners of full f32 precision at ~1e-38: mode 0 knows each of them to within 2^-134, so an
    output may be off by that times the magnitudes it is multiplied with -- 2^-134 * 3.0e38 = 0.014 in row ROW, nothing
    measurable elsewhere -- on top of the usual bound, and by no more.  Mode 1 multiplies them as f32 and meets both bounds."""
    vals = _top_of_range_values(case, 3.0e38, on_grid=False)
    sum_a = vals.a.double().abs().sum(dim=1 if case.kind == "nt" else 0)          # per output row
    sum_b = vals.b.double().abs().sum(dim=1 if case.kind == "nt" else 0)          # per output column
    allowance = 2.0 ** -134 * (sum_a[:, None] + sum_b[None, :])
    ops = Operands(case, vals, DEV)
    _lib.check(run_library(case, ops), _id(case))
    worst = check_output(case, ops, vals.ref, vals.mag, allowance=allowance)
    print(f"{_id(case)}: mode 0 with full-precision partners at 1e-38: worst error {worst:.0f} * 2^-24 * |A|.|B|")
    native = case._replace(mode=1)
    ops = Operands(native, vals, DEV)
    _lib.check(run_library(native, ops), _id(native))
    check_output(native, ops, vals.ref, vals.mag)


@pytest.mark.gpu
@pytest.mark.parametrize("big", [BF16_OVERFLOW, 3.4e38, torch.finfo(torch.float32).max])
@pytest.mark.parametrize("case", TOP_CASES, ids=_id)
def test_gemm_split_domain_ends_where_bf16_overflows(case, big):
    """An element in [3.3962e38, FLT_MAX] is outside the domain of mode 0: every output it feeds is non-finite (never a finite
    wrong value), every other output meets the bounds, and mode 1 returns the finite f32 product of the same data."""
    vals = _top_of_range_values(case, big, on_grid=False)
    assert math.isfinite(float(vals.a.abs().max())) and float(vals.a.abs().max()) >= BF16_OVERFLOW
    ops = Operands(case, vals, DEV)
    _lib.check(run_library(case, ops), _id(case))
    check_output(case, ops, vals.ref, vals.mag, poisoned_rows=(ROW,))
    native = case._replace(mode=1)
    ops = Operands(native, vals, DEV)
    _lib.check(run_library(native, ops), _id(native))
    check_output(native, ops, vals.ref, vals.mag)


# ===================================================================================================== no GPU from here on
@pytest.mark.parametrize("case", NT_CASES + TN_CASES + TOP_CASES, ids=_id)
def test_cases_reach_the_kernels_they_name(case):
    got = nt_dispatch(case) if case.kind == "nt" else tn_dispatch(case)
    assert {k: got[k] for k in case.expect} == case.expect, got
    assert case.k <= 2048 or (case.kind == "tn" and _cdiv(case.k, tn_slabs(case.m, case.n, case.k)) <= 2048)


def test_case_list_covers_every_kernel_and_epilogue():
    nt, tn = [nt_dispatch(c) for c in NT_CASES], [tn_dispatch(c) for c in TN_CASES]
    assert {d["kernel"] for d in nt} >= {UNALIGNED_NT, F32_NT_64, F32_NT_128, X6_64, X6_128x256}
    assert {d["epilogue"] for d in nt if d["kernel"].startswith("gemm_nt_x6")} == {"staged", "scalar", "atomic"}
    assert {(d["kernel"], d["xcd"]) for d in nt} >= {(X6_64, True), (X6_128x256, True), (X6_128x256, False)}
    assert {d["kernel"] for d in tn} == {UNALIGNED_TN, F32_TN, X6P_TN}
    assert {(d["kernel"], d["xcd"]) for d in tn} >= {(X6P_TN, True), (X6P_TN, False)}
    assert sum(c.bias for c in NT_CASES) in range(len(NT_CASES) // 2 - 2, len(NT_CASES) // 2 + 3)


def _window(buf, at, rows, cols, ld):
    return buf.as_strided((rows, cols), (ld, 1), at)


def run_torch(c, ops, one_more=0, write_column_n=False, bias_in_every_split=False):
    """The same call on the flat CPU buffers in plain torch, honouring the leading dimensions and the base offsets.
    The three switches are the mistakes the harness exists to catch:
      one_more = 1           the reduction runs one index too far (NT: K + 1 elements of every row; TN: R + 1 rows)
      write_column_n         every row of C gets a column N
      bias_in_every_split    K is split in four and each part adds the bias"""
    if c.kind == "nt":
        a = _window(ops.a_buf, ops.a_at, c.m, c.k + one_more, c.lda).double()
        b = _window(ops.b_buf, ops.b_at, c.n, c.k + one_more, c.ldb).double()
        parts = 4 if (bias_in_every_split and c.k >= 4) else 1
        out = torch.zeros(c.m, c.n, dtype=torch.float64)
        for ka in torch.arange(c.k + one_more).chunk(parts):
            out += a[:, ka] @ b[:, ka].t()
            if ops.bias is not None and (bias_in_every_split or int(ka[0]) == 0):
                out += ops.bias.double()
    else:
        a = _window(ops.a_buf, ops.a_at, c.k + one_more, c.m, c.lda).double()
        b = _window(ops.b_buf, ops.b_at, c.k + one_more, c.n, c.ldb).double()
        out = a.t() @ b
    if write_column_n:
        ops.c_buf[ops.c_at + torch.arange(c.m) * c.ldc + c.n] = 7.0
    ops.c.copy_(out.float())


SELF_TEST_WRONG_BELOW = 1 << 20      # the wrong implementations run on the cases with fewer outputs than this (all but four)


@pytest.mark.parametrize("case", NT_CASES + TN_CASES, ids=_id)
def test_harness_accepts_a_plain_implementation_and_rejects_three_wrong_ones(case):
    vals = values_of(case)
    ops = Operands(case, vals, "cpu")
    run_torch(case, ops)
    check_output(case, ops, vals.ref, vals.mag)
    if case.m * case.n >= SELF_TEST_WRONG_BELOW:
        return
    wrong = [dict(one_more=1), dict(write_column_n=True)] + ([dict(bias_in_every_split=True)] if case.bias and case.k >= 4 else [])
    for mistake in wrong:
        ops = Operands(case, vals, "cpu")
        run_torch(case, ops, **mistake)
        with pytest.raises(AssertionError):
            check_output(case, ops, vals.ref, vals.mag)


def test_harness_rejects_an_output_left_untouched_and_a_finite_value_in_a_poisoned_row():
    case = TOP_CASES[0]
    vals = _top_of_range_values(case, 3.4e38, on_grid=False)
    ops = Operands(case, vals, "cpu")
    with pytest.raises(AssertionError):
        check_output(case, ops, vals.ref, vals.mag)               # nothing written: NaN inside the window
    run_torch(case, ops)
    check_output(case, ops, vals.ref, vals.mag)                   # the f32 product is finite and right
    with pytest.raises(AssertionError):
        check_output(case, ops, vals.ref, vals.mag, poisoned_rows=(ROW,))
    ops.c[ROW] = float("inf")
    check_output(case, ops, vals.ref, vals.mag, poisoned_rows=(ROW,))
    ops.c[ROW, 5] = 1.0
    with pytest.raises(AssertionError):
        check_output(case, ops, vals.ref, vals.mag, poisoned_rows=(ROW,))
