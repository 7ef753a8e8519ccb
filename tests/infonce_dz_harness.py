"""Shared harness of tests/test_infonce_dz_q_gpu.py and tests/test_infonce_dz_q_domain_{gpu,cpu}.py: the criterion's linear C
entries (cpc_infonce_forward + cpc_infonce_backward) run on the same inputs with CPC_NCE_DZ=rows (contribution rows, the default
path) and CPC_NCE_DZ=q (per-row context sums: infonce_bwd_fused_kernel<.., false>, infonce_dz_q_kernel, dz = Q . wq^T), the
checks both files make on the pair, the table of shapes of the domain files and the restatement of the predicate that selects
the path.  Nothing here needs a GPU to be imported; _backward and _check do to be called."""
from collections import namedtuple

import numpy as np
import torch

from cpc2_amd import _lib
from oracle import cpc_oracle as O
from oracle import synth

DEV = "cuda:0"
GUARD = 4096                # bytes of GUARD_BYTE behind `saved` and `scratch`: nothing may write past what the library asked for
GUARD_BYTE = 0xA5
NCE_POS = NCE_ROWS = 16     # csrc/infonce.hip: positive-tile columns, prediction rows of the MFMA tile
NCE_SROW = 68               # staging tile row of infonce_bwd_fused_kernel
NCE_SORT_MAX = 512          # nce_sort_kernel: longer reference lists stay in the order the atomics filled them in


# ----------------------------------------------------------------------------- which path a shape selects
def fused_ok(k, henc, nn):
    """nce_fused_ok (csrc/infonce.hip) restated: the shapes of infonce_bwd_fused_kernel."""
    lw = -(-(NCE_POS + nn) // 32) * 32 + 4
    return henc in (256, 512) and lw <= 320 and nn % 16 == 0 and k * (nn + 1) <= (henc // 128) * 16 * NCE_SROW


def q_domain(b, t_len, k, har, henc, nn):
    """nce_dz_q_wanted (csrc/infonce.hip) restated, CPC_NCE_DZ=q given: True where cpc_infonce_backward takes the per-row sums."""
    small = b > 0 and t_len > k and b * t_len * har < 2 ** 31 and b * (t_len - k) * (NCE_POS + nn) * NCE_ROWS < 2 ** 31
    return small and fused_ok(k, henc, nn) and har in (256, 512)


# ----------------------------------------------------------------------------- the shapes of the domain files
# inside: the intended side of q_domain (tests/test_infonce_dz_q_domain_cpu.py holds the table to the predicate and the predicate to
# the library's scratch sizes).  c_w: c (and dc) hold W = T - K frames per window.  floor: the rows path's own error may be next
# to nothing (one term per contribution row), so the tight gate's bound has the floor 2^-22 max|dz|.
Case = namedtuple("Case", "name b t k har henc nn inside c_w floor seed")


def _c(name, b, t, k, har, henc, nn, inside=True, c_w=False, floor=False, seed=0):
    return Case(name, b, t, k, har, henc, nn, inside, c_w, floor, seed)


CASES = (
    # every step-count class (NKK = ceil(K / 4) = 1..4, both parities; K = 5 / 13: 39 / 63 z rows, the last workgroup's spare wave)
    [_c(f"steps-K{k}-h256", 3, k + 8, k, 256, 256, 16, floor=k == 1, seed=1000 + k) for k in (1, 4, 5, 8, 9, 13, 16)]
    + [_c(f"steps-K{k}-h512", 3, k + 8, k, 512, 512, 16, floor=k == 1, seed=1100 + k) for k in (1, 13, 16)]
    # one target frame: W = 1, 13 z rows, every positive slot has exactly one entry
    + [_c("one-frame", 1, 13, 12, 256, 256, 16, floor=True, seed=1200)]
    # unequal widths
    + [_c(f"widths-{har}-{henc}-K{k}", 2, k + 8, k, har, henc, 32, seed=1300 + k + har // 256)
       for har, henc in ((256, 512), (512, 256)) for k in (12, 16)]
    # corners of the candidate (lw <= 320) and staging (K (Nneg + 1) <= (Henc / 128) 16 68) limits
    + [_c(f"corner-h{h}-K{k}-n{nn}", 2, k + 8, k, h, h, nn, seed=1400 + k + nn)
       for h, k, nn in ((256, 16, 128), (256, 12, 176), (256, 8, 256), (512, 16, 256), (512, 15, 272))]
    # c_frames = W
    + [_c("cw-base", 3, 20, 12, 256, 256, 16, c_w=True, seed=1500), _c("cw-widths-256-512", 2, 20, 12, 256, 512, 32, c_w=True, seed=1510)]
    # just outside the domain: under `q` these take the contribution rows
    + [_c("out-staging-h256-K16-n144", 2, 24, 16, 256, 256, 144, inside=False, seed=1600),
       _c("out-n24", 2, 20, 12, 256, 256, 24, inside=False, seed=1610),
       _c("out-n288", 2, 12, 4, 256, 256, 288, inside=False, seed=1620),       # (K = 4: 4 x 289 is within the staging tiles)
       _c("out-har128", 2, 20, 12, 128, 256, 16, inside=False, seed=1630),
       _c("out-henc128", 2, 20, 12, 256, 128, 16, inside=False, seed=1640)]
)
CASE_BY_NAME = {cs.name: cs for cs in CASES}
assert len(CASE_BY_NAME) == len(CASES)
# the shapes of the single tests: loss gradients with a zero and a negative entry, a window at the floor weight (K = 5), the
# module-predictor entries, the criterion module
DLOSSES = _c("dlosses", 3, 20, 12, 256, 256, 16, seed=1800)
FLOOR_WEIGHT = _c("floor-weight-K5", 3, 13, 5, 256, 256, 16, seed=1810)
PRED = _c("pred", 2, 20, 12, 256, 256, 16, seed=1820)
MODULE = _c("module", 3, 40, 12, 256, 256, 32, seed=1830)

# the reference-list case: b = 2 windows of 140 frames, K = 12, 16 negatives -> 4096 references over 280 z rows
LISTS = _c("lists", 2, 140, 12, 256, 256, 16, seed=1700)
# z row -> the length of its reference list.  Row 0 is frame 0 of window 0: negatives only (no step has frame 0 as its positive);
# row 50 has its 12 positives and no negative reference; rows 3 / 275 / 279 have 3 / 12 - 7 / 1 positives (k1 = tp - 1 < K - 1,
# k0 = tp - W > 0); row 130's list is longer than NCE_SORT_MAX.  LISTS_DEAD (frame 0 of window 1) has no reference of either kind.
LISTS_LENGTHS = {50: 0, 141: 1, 0: 7, 20: 8, 139: 9, 3: 63, 275: 64, 279: 65, 200: 128, 130: 600}
LISTS_DEAD = 140


def lists_ext(case=LISTS, lengths=None, dead=LISTS_DEAD, seed=17):
    """The constructed negatives of the reference-list case, in negative_indices' [b, n_neg, W] order: the rows of `lengths`
    receive exactly that many references, `dead` none, the rest of the b W n_neg references go to the other rows at random."""
    lengths = LISTS_LENGTHS if lengths is None else lengths
    b, t_len, w_len, nn = case.b, case.t, case.t - case.k, case.nn
    total = b * nn * w_len
    named = np.concatenate([np.full(n, r, dtype=np.int64) for r, n in lengths.items()])
    others = np.array([r for r in range(b * t_len) if r not in lengths and r != dead], dtype=np.int64)
    rs = np.random.RandomState(seed)
    fill = others[rs.randint(0, len(others), size=total - len(named))]
    return rs.permutation(np.concatenate([named, fill])).reshape(b, nn, w_len)


def list_lengths(ext, rows):
    """Length of every z row's reference list."""
    return np.bincount(np.asarray(ext).reshape(-1), minlength=rows)


def unsorted_rows(ext, rows):
    """The z rows whose list nce_sort_kernel leaves as filled: the order of their sum, hence dz's last bits, is not promised."""
    return list_lengths(ext, rows) > NCE_SORT_MAX


def dead_rows(ext, b, t_len):
    """z rows nobody refers to: no negative, and frame 0 of a window is no step's positive (the positive of step k at t is frame
    t + 1 + k).  (T > K: every later frame is the positive of some step.)"""
    referred = np.zeros(b * t_len, dtype=bool)
    referred[np.asarray(ext).reshape(-1)] = True
    referred.reshape(b, t_len)[:, 1:] = True
    return ~referred


# ----------------------------------------------------------------------------- inputs
def _random_ext(b, t_len, nn, seed, rows=None, k=12):
    """Negatives in negative_indices' [b, n_neg, W] order (int64, flat), drawn uniformly from `rows` (default: every z row)."""
    rs = np.random.RandomState(seed)
    rows = np.arange(b * t_len) if rows is None else np.asarray(rows)
    return rows[rs.randint(0, len(rows), size=(b, nn, t_len - k))].astype(np.int64)


def _time_major(ext, b, w_len, nn):
    return torch.as_tensor(np.asarray(ext).reshape(b, nn, w_len).transpose(0, 2, 1).copy(), dtype=torch.int32)


def _inputs(b, t_len, h, seed, k=12, henc=None, c_frames=None):
    """c [b, c_frames, h] (default: T frames; W = T - K: the first W of the same), z [b, T, henc] (default h), the K predictors
    [henc, h]."""
    henc = h if henc is None else henc
    cp = synth.predictor_params(k, h, henc, seed=seed, scale=2.0)
    wk = [cp[f"wPrediction.predictors.{i}.weight"] for i in range(k)]
    c = synth.features((b, t_len, h), seed + 1)
    if c_frames is not None and c_frames != t_len:
        assert c_frames == t_len - k
        c = c[:, :c_frames].contiguous()
    return c, synth.features((b, t_len, henc), seed + 2, relu=True), wk


def default_dlosses(k, dtype=torch.float32):
    return torch.linspace(0.5, 1.5, k, dtype=dtype)


# ----------------------------------------------------------------------------- the two paths
def _scratch_need(monkeypatch, lib, mode, b, t_len, k, dim_ar, henc, nn):
    monkeypatch.setenv("CPC_NCE_DZ", mode)
    return lib.cpc_infonce_scratch_bytes(b, t_len, k, dim_ar, henc, nn)


def _guarded(nbytes, fill=None):
    """nbytes + GUARD bytes on the device, the last GUARD of them GUARD_BYTE."""
    buf = torch.empty(nbytes + GUARD, dtype=torch.uint8, device=DEV) if fill is None else \
        torch.full((nbytes + GUARD,), fill, dtype=torch.uint8, device=DEV)
    buf[nbytes:] = GUARD_BYTE
    return buf


def _backward(mode, monkeypatch, c, z, wk, ext, nn, weights, launches=1, dlosses=None):
    """cpc_infonce_forward + cpc_infonce_backward (immediate form) with CPC_NCE_DZ = mode, K = len(wk) steps, widths and the
    context's frames per window (T or W) as the tensors have them: per launch on the same inputs (dc, dz, dW, dP, losses).
    `saved` and `scratch` are followed by GUARD bytes that no launch may touch."""
    monkeypatch.setenv("CPC_NCE_DZ", mode)
    lib = _lib.load()
    k = len(wk)
    henc, h = wk[0].shape
    b, t_len, _ = z.shape
    c_frames = c.shape[1]
    w_len = t_len - k
    assert z.shape[2] == henc and c.shape == (b, c_frames, h) and c_frames in (t_len, w_len)
    cd, zd, wpred = c.to(DEV), z.to(DEV), torch.stack(wk).to(DEV)
    ext_tm = _time_major(ext, b, w_len, nn).to(DEV)
    wd = None if weights is None else weights.float().to(DEV)
    dl = (default_dlosses(k) if dlosses is None else dlosses.float()).to(DEV)
    st = _lib.stream_ptr(cd.device)
    nsaved = lib.cpc_infonce_saved_bytes(b, t_len, k, h, henc, nn)
    saved = _guarded(nsaved)
    nscr = lib.cpc_infonce_scratch_bytes(b, t_len, k, -h, henc, nn)       # (the linear entries' own need, path by path)
    full = lib.cpc_infonce_scratch_bytes(b, t_len, k, h, henc, nn)
    assert nsaved > 0 and 0 < nscr <= full
    if mode == "q":
        rows_bytes = _scratch_need(monkeypatch, lib, "rows", b, t_len, k, -h, henc, nn)
        monkeypatch.setenv("CPC_NCE_DZ", "q")
        if not q_domain(b, t_len, k, h, henc, nn):
            assert rows_bytes == nscr, "outside the per-row sums' domain the linear entries' scratch need depends on CPC_NCE_DZ"
        else:
            assert rows_bytes != nscr, "the per-row sums were not selected: the scratch need is that of the contribution rows"
            if h == henc:
                # the contribution rows [b W][16 + n_neg][H] are gone from it (Q, [b T][K][H], and the re-laid predictors take their
                # place)
                assert rows_bytes - nscr >= 4 * h * (b * w_len * (16 + nn) - b * t_len * k - k * h) - 4096
    losses, acc = torch.empty(k, device=DEV), torch.empty(k, device=DEV)
    outs = []
    for _ in range(launches):
        scr = _guarded(nscr, fill=0xFF)                                   # (NaN patterns: nothing may be read before it is written)
        _lib.check(lib.cpc_infonce_forward(_lib.ptr(cd), _lib.ptr(zd), _lib.ptr(wpred), _lib.ptr(ext_tm), _lib.ptr(wd), _lib.ptr(losses),
                                           _lib.ptr(acc), _lib.ptr(saved), _lib.ptr(scr), b, t_len, c_frames, k, h, henc, nn, st), "fwd")
        dc, dz, dw = torch.full_like(cd, float("nan")), torch.full_like(zd, float("nan")), torch.full_like(wpred, float("nan"))
        _lib.check(lib.cpc_infonce_backward(_lib.ptr(cd), _lib.ptr(zd), _lib.ptr(wpred), _lib.ptr(ext_tm), _lib.ptr(wd), _lib.ptr(dl),
                                            _lib.ptr(saved), _lib.ptr(scr), _lib.ptr(dc), _lib.ptr(dz), _lib.ptr(dw), b, t_len, c_frames, k, h,
                                            henc, nn, 0, st), "bwd")
        torch.cuda.synchronize()
        _lib.check(lib.cpc_async_error_check(st), "async errors")
        for name, buf, n in (("saved", saved, nsaved), ("scratch", scr, nscr)):
            assert bool((buf[n:] == GUARD_BYTE).all()), f"{mode}: the {GUARD} bytes behind the {n} of `{name}` were written"
        # dP [b T][K Henc] (its first b c_frames rows are in use) sits behind the two [b W][K] loss / hit planes of the scratch
        # layout (256-byte carves: nce_layout)
        plane = -(-(b * w_len * k * 4) // 256) * 256
        dp = scr[2 * plane:2 * plane + 4 * b * c_frames * k * henc].view(torch.float32).clone()
        outs.append((dc, dz, dw, dp, losses.clone()))
    return outs


def _check(monkeypatch, b, t_len, h, nn, ext, seed, weights=None, k=12, henc=None, c_frames=None, dlosses=None, factor=2.0,
           floor=False, unsorted=0, structural=False, tag=None):
    """One set of inputs through both paths.  dc, dP and dW_k are bit-identical between them; two launches of the sums give the
    same dz bit for bit (but for the `unsorted` rows whose list is longer than NCE_SORT_MAX: exactly that many); z rows nobody
    refers to are exactly zero on both; against the fp64 oracle the sums' maximum element error of dz is at most `factor` times the
    contribution rows' own (floor: or 2^-22 max|dz|, where that error is next to nothing).  Outside the sums' domain (q_domain) dz
    is bit-identical as well.  structural: losses, dc, dz and dW of both paths are held to the oracle at the suite's bounds for the
    default path (1e-5, 1e-4, 1e-4, 2e-4 of the largest element).  Returns the number of z rows without a reference."""
    henc = h if henc is None else henc
    c, z, wk = _inputs(b, t_len, h, seed, k=k, henc=henc, c_frames=c_frames)
    inside = q_domain(b, t_len, k, h, henc, nn)
    rows = _backward("rows", monkeypatch, c, z, wk, ext, nn, weights, dlosses=dlosses)[0]
    new, again = _backward("q", monkeypatch, c, z, wk, ext, nn, weights, launches=2, dlosses=dlosses)
    for name, a, bb in zip(("dc", "dz", "dW", "dP", "losses"), rows, new):
        if name != "dz" or not inside:
            assert torch.equal(a, bb), f"{name} differs between the two dz paths"
    keep = torch.as_tensor(~unsorted_rows(ext, b * t_len))
    assert int((~keep).sum()) == unsorted, f"{int((~keep).sum())} reference lists are longer than NCE_SORT_MAX (expected {unsorted})"
    assert torch.equal(new[1].cpu().view(b * t_len, henc)[keep], again[1].cpu().view(b * t_len, henc)[keep]), \
        "dz differs between two launches on the same inputs"
    dl64 = default_dlosses(k, torch.float64) if dlosses is None else dlosses.double()
    ref = O.criterion_forward_sparse(c.double(), z.double(), [w.double() for w in wk], np.asarray(ext).reshape(-1), nn, weights=weights,
                                     dlosses=dl64)
    ref_dz = ref["dz"]
    top = float(ref_dz.abs().max())
    assert top > 0
    err_rows = float((rows[1].cpu().double() - ref_dz).abs().max())
    err_new = float((new[1].cpu().double() - ref_dz).abs().max())
    print(f"dz {tag or ''} b{b} T{t_len} K{k} Har{h} Henc{henc} n{nn} c_frames {c.shape[1]}: max element error rows path {err_rows:.3e}, "
          f"per-row sums {err_new:.3e}, ratio {err_new / max(err_rows, 1e-300):.2f} (max |dz| {top:.3e}, 2^-22 of it {top * 2.0 ** -22:.3e})")
    dead = torch.as_tensor(dead_rows(ext, b, t_len))
    for name, dz in (("rows", rows[1]), ("per-row sums", new[1])):
        assert bool((dz.cpu().view(b * t_len, henc)[dead] == 0).all()), f"{name}: a z row without a reference is not zero"
    if structural:
        for path, out in (("rows", rows), ("per-row sums", new)):
            for name, got, want, tol in (("losses", out[4], ref["losses"].view(-1), 1e-5), ("dc", out[0], ref["dc"], 1e-4),
                                         ("dz", out[1], ref_dz, 1e-4), ("dW", out[2], torch.stack(ref["dW"]), 2e-4)):
                err = float((got.cpu().double() - want).abs().max())
                assert err <= tol * float(want.abs().max()), f"{path}: {name} is {err:.3e} from the fp64 oracle (largest {float(want.abs().max()):.3e})"
    bound = factor * err_rows
    if floor:
        bound = max(bound, 2.0 ** -22 * top)
    assert err_new <= bound, (f"dz error {err_new:.3e} against the fp64 oracle exceeds {factor} x the rows path's {err_rows:.3e}"
                              + (f" and 2^-22 max|dz| = {2.0 ** -22 * top:.3e}" if floor else ""))
    return int(dead.sum())
