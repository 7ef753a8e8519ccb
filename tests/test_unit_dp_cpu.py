"""Duration-penalized unit segmentation without a GPU: the numpy oracle (unit_dp_oracle.py) against brute force over every labeling,
properties of the minimiser on random real costs, the tie rules on hand-made cases, cpc2_amd.unit_segmentation.runs, the refusals of
the segment_quantization tool raised before a file of audio is opened, and the C entry points' refusals that need no device."""
import builtins
import json
import os
import re

import numpy as np
import pytest

import unit_dp_oracle as DO
from cpc2_amd import _lib
from cpc2_amd import unit_segmentation as seg
from cpc2_amd.clustering import segment_quantization as sq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- the oracle against brute force
def test_oracle_against_brute_force():
    """Integer costs in [0, 7] and integer penalties: every V is an exact integer, so == holds.  Every (T, K) with T <= 6, K <= 3,
    every penalty of {0, 1, 3, 50}, 4 seeded cost matrices each: 6 * 3 * 4 * 4 = 288 cases."""
    rs = np.random.RandomState(0)
    cases = 0
    for T in range(1, 7):
        for K in range(1, 4):
            for lam in (0, 1, 3, 50):
                for _ in range(4):
                    cost = rs.randint(0, 8, size=(T, K)).astype(np.float32)
                    u, energy, n_seg, status = DO.segment(cost, lam)
                    assert status == DO.DONE
                    best = DO.brute_force(cost, lam)
                    assert energy == best, (T, K, lam, cost)
                    assert DO.labeling_energy(cost, u, lam) == best, (T, K, lam, cost, u)      # its own labeling attains it
                    assert n_seg == 1 + int((u[1:] != u[:-1]).sum())
                    cases += 1
    assert cases == 288


# ----------------------------------------------------------------------------- properties on random real costs
@pytest.mark.parametrize("seed", range(6))
def test_segments_do_not_increase_with_the_penalty(seed):
    rs = np.random.RandomState(10 + seed)
    T, K = int(rs.randint(20, 200)), int(rs.randint(2, 40))
    cost = (rs.rand(T, K) * 10).astype(np.float32)
    counts = [DO.segment(cost, lam)[2] for lam in (0.0, 0.01, 0.1, 0.5, 1.0, 2.0, 5.0, 20.0, 1e3)]
    assert all(a >= b for a, b in zip(counts, counts[1:])), counts
    assert counts[0] > counts[-1] == 1


@pytest.mark.parametrize("seed", range(6))
def test_large_penalty_gives_the_best_single_unit(seed):
    rs = np.random.RandomState(20 + seed)
    T, K = int(rs.randint(2, 120)), int(rs.randint(1, 30))
    cost = (rs.randn(T, K) * 3).astype(np.float32)
    c = cost.astype(np.float64)
    lam = float((c.max(axis=1) - c.min(axis=1)).sum()) + 1.0            # above sum_t (max_k c - min_k c)
    u, energy, n_seg, _ = DO.segment(cost, lam)
    sums = np.zeros(K)
    for t in range(T):                                                   # the column sums in the chain's order
        sums = sums + c[t]
    assert n_seg == 1 and (u == int(np.argmin(sums))).all() and energy == sums.min()


@pytest.mark.parametrize("seed", range(4))
def test_zero_penalty_on_integer_costs_is_the_framewise_argmin(seed):
    """lambda = 0: V[t] = c[t] + m[t-1], so every u[t] is a frame-wise minimum and the energy is their sum.  Where a frame has ONE
    minimum it is the argmin.  Where it has several, `a tie stays` decides: the unit of frame t + 1 is kept when it is among them,
    otherwise the lowest index is taken -- so the stream is NOT the lowest-index argmin of every frame, but exactly this rule."""
    rs = np.random.RandomState(30 + seed)
    cost = rs.randint(0, 6, size=(80, 7)).astype(np.float32)            # many equal minima
    u, energy, _, _ = DO.segment(cost, 0.0)
    low = cost.min(axis=1)
    assert energy == low.sum() and (cost[np.arange(80), u] == low).all()
    want = np.zeros(80, np.int64)
    want[79] = cost[79].argmin()
    for t in range(78, -1, -1):
        want[t] = want[t + 1] if cost[t, want[t + 1]] == low[t] else cost[t].argmin()
    assert np.array_equal(u, want)
    assert (want != cost.argmin(axis=1)).any()                           # (the rule does differ from the plain argmin here)
    single = (cost == low[:, None]).sum(axis=1) == 1
    assert single.sum() > 10 and np.array_equal(u[single], cost.argmin(axis=1)[single])
    # one minimum in every frame: the lowest-index argmin and nothing else
    perm = np.stack([rs.permutation(7) for _ in range(80)]).astype(np.float32)
    u, energy, _, _ = DO.segment(perm, 0.0)
    assert np.array_equal(u, perm.argmin(axis=1)) and energy == 0.0


# ----------------------------------------------------------------------------- tie rules
def test_equal_minima_resolve_to_the_lowest_index():
    cost = np.array([[2, 1, 1, 1], [5, 5, 5, 5]], dtype=np.float32)
    u, energy, n_seg, _ = DO.segment(cost, 1.0)
    assert u.tolist() == [1, 1] and energy == 6.0 and n_seg == 1
    u, _, _, _ = DO.segment(np.array([[3, 3, 3]], dtype=np.float32), 0.0)
    assert u.tolist() == [0]


def test_stay_wins_a_tie_with_the_switch():
    """V[0] = (0, 2), lambda = 2: sw = 2 == V[0][1], state 1 stays.  Frame 1 makes state 1 the minimum: its predecessor is itself,
    although switching from state 0 costs the same."""
    cost = np.array([[0, 2], [9, 0]], dtype=np.float32)
    u, energy, n_seg, _ = DO.segment(cost, 2.0)
    assert u.tolist() == [1, 1] and energy == 2.0 and n_seg == 1
    u, energy, n_seg, _ = DO.segment(cost, 1.5)                         # a cheaper switch is taken
    assert u.tolist() == [0, 1] and energy == 1.5 and n_seg == 2


def test_negative_zero_equals_positive_zero():
    cost = np.array([[0.0, -0.0], [-0.0, 0.0], [1.0, 1.0]], dtype=np.float32)
    u, energy, n_seg, _ = DO.segment(cost, 0.0)
    assert u.tolist() == [0, 0, 0] and energy == 1.0 and n_seg == 1
    u, _, _, _ = DO.segment(np.array([[-0.0, 0.0]], dtype=np.float32), 0.0)
    assert u.tolist() == [0]


def test_statuses_of_the_oracle_pack():
    cost = np.arange(24, dtype=np.float32).reshape(8, 3)
    cost[6, 1] = np.inf
    units, energy, n_seg, status = DO.segment_pack(cost, [0, 3, 6, 7, -1, 2], [3, 0, 2, 2, 2, 3], [0.0, 4.0])
    assert status.tolist() == [[0, 1, 2, 3, 3, 0]] * 2
    assert units[0].tolist() == [0, 0, 0, 0, 0, -2, -1, -1] and energy[0, 1] == 0 and np.isnan(energy[0, 2]) and np.isnan(energy[0, 3])


# ----------------------------------------------------------------------------- runs
def test_runs():
    units = np.array([7, 7, 3, 3, 3, 9, -5, 4, 4], dtype=np.int32)
    out = seg.runs(units, [0, 7, 6, 8, 20], [6, 2, 0, 1, 3])
    assert [o.tolist() for o in out[0]] == [[7, 3, 9], [0, 2, 5], [2, 3, 1]]
    assert [o.tolist() for o in out[1]] == [[4], [0], [2]]
    assert [o.tolist() for o in out[2]] == [[], [], []] and [o.tolist() for o in out[4]] == [[], [], []]
    assert [o.tolist() for o in out[3]] == [[4], [0], [1]]
    with pytest.raises(ValueError, match="one row"):
        seg.runs(np.zeros((2, 3), np.int32), [0], [3])


def test_penalties_are_checked_on_the_host():
    assert seg.check_penalties([0, 2.5]) == [0.0, 2.5] and seg.check_penalties(3) == [3.0]
    for bad in ([], [0.0] * 17, [-1.0], [float("nan")], [float("inf")]):
        with pytest.raises(ValueError, match="penalt"):
            seg.check_penalties(bad)


def test_segment_costs_refuses_host_tensors():
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        seg.segment_costs(torch.zeros(4, 3), [0], [4], [1.0])


# ----------------------------------------------------------------------------- the tool's refusals
MISSING = os.path.join(ROOT, "no", "such", "place")
BASE = [os.path.join(MISSING, "checkpoint_last.pt"), MISSING]
REFUSED = [
    (BASE + [ROOT, "--penalty", "1"], ValueError, "OUT_DIR .* not an empty directory"),
    (BASE + [MISSING, "--penalty", "-1"], ValueError, "--penalty -1.0"),
    (BASE + [MISSING, "--penalty", "nan"], ValueError, "--penalty nan"),
    (BASE + [MISSING, "--penalty", "1", "inf"], ValueError, "--penalty inf"),
    (BASE + [MISSING, "--penalty", "1", "2", "1.0"], ValueError, "--penalty .* repeated"),
    (BASE + [MISSING, "--penalty"] + [str(i) for i in range(17)], ValueError, "--penalty: 17 values"),
    (BASE + [MISSING, "--penalty", "1", "--file_extension", ".mp3"], NotImplementedError, "--file_extension .mp3"),
    (BASE + [MISSING, "--penalty", "1", "--separate-speaker"], NotImplementedError, "--separate-speaker"),
]


def _watch(monkeypatch):
    opened = []
    real_open = builtins.open

    def watched(file, *a, **k):
        opened.append(str(file))
        return real_open(file, *a, **k)

    monkeypatch.setattr(builtins, "open", watched)
    monkeypatch.setattr(sq, "findAllSeqs", lambda *a, **k: opened.append("findAllSeqs") or ([], []))
    return opened


@pytest.mark.parametrize("argv,error,text", REFUSED, ids=[f"#{i} " + r[2] for i, r in enumerate(REFUSED)])
def test_tool_refuses_before_a_file_is_opened(argv, error, text, monkeypatch):
    opened = _watch(monkeypatch)
    with pytest.raises(error, match=text):
        sq.main(argv)
    assert not opened and not os.path.exists(MISSING)


@pytest.mark.parametrize("run_args,text", [({"dimReduction": "pca.pt", "nGroups": 1}, "--dimReduction"),
                                           ({"dimReduction": None, "nGroups": 2}, "nGroups = 2")])
def test_tool_refuses_a_clustering_run_it_cannot_segment(run_args, text, tmp_path, monkeypatch):
    """These two need the run's args.json and nothing else: no checkpoint exists and the audio directory is never listed."""
    with open(tmp_path / "args.json", "w") as f:
        json.dump(run_args, f)
    opened = _watch(monkeypatch)
    with pytest.raises(NotImplementedError, match=text):
        sq.main([str(tmp_path / "checkpoint_last.pt"), MISSING, MISSING, "--penalty", "0", "1"])
    assert opened == [str(tmp_path / "args.json")] and not os.path.exists(MISSING)


# ----------------------------------------------------------------------------- the C ABI, host side
def test_entry_points_are_declared_and_sized():
    header = open(os.path.join(ROOT, "include", "cpc2_hip.h")).read()
    assert "V[t][k] = (double) c[t][k] + (stay[t][k] ? V[t-1][k] : sw) (one f64 add)" in header     # the definition, verbatim
    assert "u[t-1] = stay[t][u[t]] ? u[t] : a[t-1]" in header
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("cpc_segment_units", "cpc_segment_units_scratch_bytes", "cpc_segment_units_wave_k"):
        assert re.search(r"\b" + name + r"\s*\(", header) and name in _lib.SIGNATURES, name
    lib = _lib.load()
    assert lib.cpc_version() >= 129
    assert 64 <= lib.cpc_segment_units_wave_k() < 16384
    words = (50 + 31) // 32
    assert lib.cpc_segment_units_scratch_bytes(10, 1000, 50, 3) >= 8 * 11 + 3 * 1000 * 4 * (words + 1)
    for bad in ((-1, 10, 50, 1), ((1 << 20) + 1, 10, 50, 1), (1, -1, 50, 1), (1, 10, 0, 1), (1, 10, 16385, 1), (1, 10, 50, 0),
                (1, 10, 50, 17)):
        assert lib.cpc_segment_units_scratch_bytes(*bad) == 0 and b"segment_units" in lib.cpc_last_error(), bad
    assert seg.MAX_UNITS == 16384 and seg.MAX_PENALTIES == 16
