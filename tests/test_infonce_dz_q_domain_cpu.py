"""What tests/test_infonce_dz_q_domain_gpu.py claims about its own inputs, checked without a GPU: the table of shapes sits on the
intended side of the per-row sums' domain (tests/infonce_dz_harness.py: q_domain, a restatement of nce_dz_q_wanted that the
library's own scratch sizes are held against here), the constructed reference lists have the stated lengths, the fp64 oracle's dz
is zero exactly on the rows nobody refers to, and one row alone is left out of the bit-reproducibility check."""
import numpy as np
import pytest
import torch

from cpc2_amd import _lib
from oracle import cpc_oracle as O
from tests import infonce_dz_harness as H

_ALL = list(H.CASES) + [H.LISTS, H.DLOSSES, H.FLOOR_WEIGHT, H.PRED, H.MODULE]


@pytest.mark.parametrize("case", _ALL, ids=lambda cs: cs.name)
def test_case_is_on_the_intended_side_of_the_domain(case, monkeypatch):
    """The predicate written out in Python puts the case where the table says, and the library agrees: the linear entries' scratch
    need (dim_ar < 0) depends on CPC_NCE_DZ exactly inside the domain; the need for every entry (dim_ar > 0) covers both."""
    assert H.q_domain(case.b, case.t, case.k, case.har, case.henc, case.nn) == case.inside
    lib = _lib.load()
    need = {}
    for mode in ("rows", "q"):
        monkeypatch.setenv("CPC_NCE_DZ", mode)
        need[mode] = lib.cpc_infonce_scratch_bytes(case.b, case.t, case.k, -case.har, case.henc, case.nn)
        need[mode, "all"] = lib.cpc_infonce_scratch_bytes(case.b, case.t, case.k, case.har, case.henc, case.nn)
    monkeypatch.delenv("CPC_NCE_DZ")
    assert lib.cpc_infonce_scratch_bytes(case.b, case.t, case.k, -case.har, case.henc, case.nn) == need["rows"] > 0
    assert (need["q"] != need["rows"]) == case.inside
    assert need["rows", "all"] == need["rows"]
    assert need["q", "all"] >= max(need["q"], need["rows"])
    if case.inside:
        assert need["q", "all"] == max(need["q"], need["rows"])


def test_table_holds_what_the_gpu_file_says_it_does():
    by = H.CASE_BY_NAME
    # all four NKK = ceil(K / 4) instantiations at both widths, odd z-row counts (RPB = 2 rows per workgroup at Har 256)
    assert {-(-cs.k // 4) for cs in H.CASES if cs.inside and cs.har == cs.henc == 256} == {1, 2, 3, 4}
    assert {-(-cs.k // 4) for cs in H.CASES if cs.inside and cs.har == cs.henc == 512} == {1, 4}
    assert by["steps-K5-h256"].b * by["steps-K5-h256"].t == 39 and by["steps-K13-h256"].b * by["steps-K13-h256"].t == 63
    assert by["one-frame"].t - by["one-frame"].k == 1 and by["one-frame"].b * by["one-frame"].t == 13
    assert {(cs.har, cs.henc) for cs in H.CASES if cs.inside and cs.har != cs.henc} == {(256, 512), (512, 256)}
    assert max(cs.nn for cs in H.CASES if cs.inside) == 272
    # the corners ARE corners: one more step, or one more tile of negatives, leaves the domain
    corners = [cs for cs in H.CASES if cs.name.startswith("corner-")]
    assert len(corners) == 5
    for cs in corners:
        more_steps = cs.k < 16 and H.q_domain(cs.b, cs.t + 1, cs.k + 1, cs.har, cs.henc, cs.nn)
        more_negatives = H.q_domain(cs.b, cs.t, cs.k, cs.har, cs.henc, cs.nn + 16)
        assert not more_steps and not more_negatives, cs.name
    # outside: each case breaks ONE condition
    out = {cs.name: cs for cs in H.CASES if not cs.inside}
    assert len(out) == 5
    for cs in out.values():
        broken = [not (cs.henc in (256, 512)), not (cs.har in (256, 512)), cs.nn % 16 != 0, -(-(16 + cs.nn) // 32) * 32 + 4 > 320,
                  cs.henc in (256, 512) and cs.k * (cs.nn + 1) > (cs.henc // 128) * 16 * H.NCE_SROW]
        assert sum(broken) == 1, (cs.name, broken)


def test_constructed_lists_have_the_stated_lengths():
    cs = H.LISTS
    rows, w_len = cs.b * cs.t, cs.t - cs.k
    ext = H.lists_ext()
    assert ext.shape == (cs.b, cs.nn, w_len) and ext.dtype == np.int64 and ext.size == 4096 and rows == 280
    assert ext.min() >= 0 and ext.max() < rows
    n = H.list_lengths(ext, rows)
    assert sorted(H.LISTS_LENGTHS.values()) == [0, 1, 7, 8, 9, 63, 64, 65, 128, 600]
    for r, want in H.LISTS_LENGTHS.items():
        assert n[r] == want, (r, n[r], want)
    assert n[H.LISTS_DEAD] == 0 and H.LISTS_DEAD % cs.t == 0
    # a row with positives and no negative reference; frame 0 of a window with negatives only; positives cut at both ends
    zero = [r for r, v in H.LISTS_LENGTHS.items() if v == 0][0]
    assert zero % cs.t >= cs.k
    assert n[0] > 0
    tps = {r % cs.t for r, v in H.LISTS_LENGTHS.items() if v > 0}
    assert any(0 < tp < cs.k for tp in tps) and any(tp > w_len for tp in tps) and (cs.t - 1) in tps
    # the 600 references of one row repeat within single (b, t)s: there are only b W = 256 of those
    long_row = [r for r, v in H.LISTS_LENGTHS.items() if v == 600][0]
    per_bt = (ext == long_row).sum(axis=1)
    assert per_bt.shape == (cs.b, w_len) and per_bt.max() >= 3 and per_bt.sum() == 600
    # every other row's list is short, and no other row is without a reference
    others = np.ones(rows, dtype=bool)
    others[list(H.LISTS_LENGTHS) + [H.LISTS_DEAD]] = False
    assert n[others].min() >= 1 and n[others].max() <= 64
    # exactly one row is left out of the bit-reproducibility check, exactly one is dead
    assert np.flatnonzero(H.unsorted_rows(ext, rows)).tolist() == [long_row]
    assert np.flatnonzero(H.dead_rows(ext, cs.b, cs.t)).tolist() == [H.LISTS_DEAD]
    assert np.array_equal(ext, H.lists_ext())


def _oracle_dz(cs, ext, **kw):
    c, z, wk = H._inputs(cs.b, cs.t, cs.har, cs.seed, k=cs.k, henc=cs.henc)
    ref = O.criterion_forward_sparse(c.double(), z.double(), [w.double() for w in wk], ext.reshape(-1), cs.nn,
                                     dlosses=H.default_dlosses(cs.k, torch.float64), **kw)
    return ref["dz"].view(cs.b * cs.t, cs.henc)


def test_oracle_dz_is_zero_exactly_on_the_dead_rows():
    """fp64 oracle on the reference-list case and on the one-frame case: every referred row has a gradient, a row without a
    reference has none -- what the GPU file's `exactly zero` assertion and its comparison with the oracle lean on."""
    for cs, ext in ((H.LISTS, H.lists_ext()), (H.CASE_BY_NAME["one-frame"], None)):
        if ext is None:
            # negatives from frames 1 .. 12 only: frame 0, nobody's positive, is then dead
            ext = H._random_ext(cs.b, cs.t, cs.nn, cs.seed, rows=range(1, cs.t), k=cs.k)
        dz = _oracle_dz(cs, ext)
        dead = torch.as_tensor(H.dead_rows(ext, cs.b, cs.t))
        assert int(dead.sum()) == 1
        assert bool((dz[dead] == 0).all())
        assert bool((dz[~dead].abs().amax(dim=1) > 0).all())


def test_a_zero_loss_gradient_silences_its_step():
    """The oracle with dlosses[3] = 0: dW_3 is exactly zero, and dz is what the other eleven steps give."""
    cs = H.DLOSSES
    ext = H._random_ext(cs.b, cs.t, cs.nn, cs.seed, k=cs.k)
    c, z, wk = H._inputs(cs.b, cs.t, cs.har, cs.seed, k=cs.k)
    dl = H.default_dlosses(cs.k, torch.float64)
    dl[3], dl[7] = 0.0, -0.75
    ref = O.criterion_forward_sparse(c.double(), z.double(), [w.double() for w in wk], ext.reshape(-1), cs.nn, dlosses=dl)
    assert float(ref["dW"][3].abs().max()) == 0.0 and float(ref["dW"][7].abs().max()) > 0
    dl2 = dl.clone()
    dl2[3] = 1.0
    ref2 = O.criterion_forward_sparse(c.double(), z.double(), [w.double() for w in wk], ext.reshape(-1), cs.nn, dlosses=dl2)
    assert float((ref2["dz"] - ref["dz"]).abs().max()) > 1e-3 * float(ref["dz"].abs().max())
