#!/usr/bin/env python3
"""Generate tests/golden/g26_per.npz by running the REFERENCE's beam_search and get_seq_PER (cpc/criterion/seq_alignment.py)
on the CPU, beside the float32 trie statement of tests/per_oracle.py.

Needs a checkout of the reference repository (the directory that holds its `cpc` package):
    CPC_REFERENCE=DIR PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_per.py

The reference is imported unmodified; progressbar is stubbed.  Arrays only.  Recorded:
  * search cases (T, P, nKeep, blank): the input [T, P] float32, the reference's nKeep scores as float32 bit patterns, its label
    sequences (padded with -1) and their lengths, and whether the case is tie-free (no two equal scores among the first
    nKeep + 1 candidates of any frame, decided by per_oracle).  A case that is compared by equality must be tie-free: seeds
    0 .. 31 are tried in turn and the first tie-free one is kept; the tool fails if there is none.  On every tie-free case
    per_oracle must equal the reference, bits and labels, or the tool fails.
  * one case that must meet ties (two identical columns), and the two searches of the reference's own unit tests
    (cpc/unit_tests.py:224-261) on their inputs rounded to float32.
  * 40 random label pairs (hypothesis of 0 .. 60 labels, reference of 1 .. 60; equal sequences, an empty hypothesis and a
    hypothesis longer than the reference among them) plus the pair of cpc/unit_tests.py:269-276: NeedlemanWunschAlignScore
    unnormalised for (d, m, r) = (-1, -1, 0) and (-2, -3, 1), and get_seq_PER.
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("CPC_REFERENCE")
if not REF or not os.path.isdir(os.path.join(REF, "cpc")):
    raise SystemExit("set CPC_REFERENCE to a checkout of the reference repository (the directory that holds cpc/)")
OUT = os.path.join(ROOT, "tests", "golden")
sys.modules["progressbar"] = types.ModuleType("progressbar")
_spec = importlib.util.spec_from_file_location("ref_seq_alignment", os.path.join(REF, "cpc", "criterion", "seq_alignment.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import per_oracle  # noqa: E402

ARR = {}
META = {"search": [], "unit": []}


def rnd(T, P, seed, scale):
    g = torch.Generator().manual_seed(seed)
    return torch.softmax(scale * torch.randn(T, P, generator=g), 1).numpy()


def peaky(T, P, seed, conf=0.9):
    """One class per frame at about `conf`."""
    g = torch.Generator().manual_seed(seed)
    path = torch.randint(0, P, (T,), generator=g)
    logits = torch.randn(T, P, generator=g)
    logits[torch.arange(T), path] += float(np.log(conf / (1 - conf) * (P - 1)))
    return torch.softmax(logits, 1).numpy()


def tied(T, P, seed):
    """Columns 0 and 1 identical: the prefixes [0] and [1] score the same from the first frame on."""
    p = rnd(T, P, seed, 1.0).copy()
    p[:, 1] = p[:, 0]
    return (p / p.sum(1, keepdims=True)).astype(np.float32)


# name, maker(seed), nKeep, blank, first seed, must be tie-free
CASES = [
    ("T1P2k1", lambda s: rnd(1, 2, s, 1.0), 1, 1, 0, True),
    ("T7P3k1", lambda s: rnd(7, 3, s, 2.0), 1, 2, 0, True),
    ("T32P9k20", lambda s: rnd(32, 9, s, 2.5), 20, 8, 0, True),
    ("T32P9k20_blankmid", lambda s: rnd(32, 9, s, 2.5), 20, 3, 1, True),
    ("T40P70k20_peaky", lambda s: peaky(40, 70, s), 20, 69, 0, True),
    ("T128P42k100_peaky", lambda s: peaky(128, 42, s), 100, 41, 0, True),
    ("T96P42k20_rand", lambda s: rnd(96, 42, s, 3.0), 20, 41, 0, True),
    ("T128P42k20_rand_denormal", lambda s: rnd(128, 42, s, 3.0), 20, 41, 0, True),
    ("T6P5k4_tied", lambda s: tied(6, 5, s), 4, 4, 0, False),
]


def bits(x):
    return np.array([np.float32(v) for v in x], np.float32).view(np.uint32)


def record(tag, probs, n_keep, blank):
    out = ref.beam_search(probs, n_keep, blank)
    mine, tie = per_oracle.beam_search(probs, n_keep, blank)
    width = max(1, max(len(x[1]) for x in out))
    labels = np.full((len(out), width), -1, np.int32)
    for i, (_, lab) in enumerate(out):
        labels[i, :len(lab)] = lab
    ARR[f"{tag}_probs"] = np.ascontiguousarray(probs, np.float32)
    ARR[f"{tag}_score_bits"] = bits([x[0] for x in out])
    ARR[f"{tag}_labels"] = labels
    ARR[f"{tag}_lens"] = np.array([len(x[1]) for x in out], np.int32)
    same = len(out) == len(mine) and all(np.float32(a[0]).tobytes() == np.float32(b[0]).tobytes() and list(a[1]) == list(b[1])
                                         for a, b in zip(out, mine))
    return tie, same, float(out[0][0])


def search_cases():
    for name, make, n_keep, blank, seed0, tie_free in CASES:
        for seed in range(seed0, 32):
            probs = make(seed)
            assert probs.dtype == np.float32
            tie, same, best = record(f"bs_{name}", probs, n_keep, blank)
            if tie == (not tie_free):
                break
        else:
            raise SystemExit(f"{name}: no seed in 0 .. 31 is " + ("tie-free" if tie_free else "tied"))
        if tie_free and not same:
            raise SystemExit(f"{name}: tests/per_oracle.py differs from the reference on a tie-free case")
        T, P = probs.shape
        META["search"].append(dict(name=name, T=T, P=P, nKeep=n_keep, blank=blank, seed=seed, tie_free=not tie, best=best))
        print(f"{name}: seed {seed} tie {tie} oracle==reference {same} best {best:.3e}")


def unit_cases():
    cases = [("ut_small", np.array([[0.1, 0.2, 0.], [0.4, 0.2, 0.6], [0.01, 0.3, 0.]]), 10, 2),
             ("ut_big", np.array([[0.1, 0.2, 0., 0., 0., 0., 0., 0.01, 0., 0.1, 0.99, 0.1],
                                  [0.1, 0.2, 0.6, 0.1, 0.9, 0., 0., 0.01, 0., 0.9, 1., 0.]]), 10, 11)]
    for name, data, n_keep, blank in cases:
        probs = data.astype(np.float32)
        tie, same, best = record(name, probs, n_keep, blank)
        META["unit"].append(dict(name=name, T=probs.shape[0], P=probs.shape[1], nKeep=n_keep, blank=blank, tie_free=not tie,
                                 best=best))
        print(f"{name}: tie {tie} oracle==reference {same} best {best}")


def pairs():
    rng = np.random.default_rng(26)
    seqs = []
    for k in range(40):
        n1 = int(rng.integers(1, 61))
        n2 = int(rng.integers(0, 61))
        n_sym = int(rng.integers(2, 42))
        s1 = rng.integers(0, n_sym, n1)
        s2 = rng.integers(0, n_sym, n2)
        if k == 0:
            s2 = s1.copy()                                     # equal sequences
        elif k == 1:
            s2 = s2[:0]                                        # an empty hypothesis
        elif k == 2:
            s1, s2 = s1[:7], rng.integers(0, n_sym, 60)        # a hypothesis longer than the reference
        elif k == 3:
            s1 = rng.integers(0, n_sym, 60)
            s2 = np.delete(s1, [5, 17, 40])                    # three deletions
        elif k % 4 == 0:
            s2 = s1[:n1].copy()[:max(1, n1 - 2)]               # a near copy: substitutions and a cut
            s2[::3] = (s2[::3] + 1) % n_sym
        seqs.append((s1, s2))
    seqs.append((np.array([0, 1, 1, 2, 0, 2, 2]), np.array([1, 1, 2, 2, 0, 0])))           # cpc/unit_tests.py:269-276
    n = len(seqs)
    a = np.zeros((n, 60), np.int32)
    b = np.zeros((n, 60), np.int32)
    la, lb = np.zeros(n, np.int32), np.zeros(n, np.int32)
    s110, s231, per = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.float64)
    for i, (s1, s2) in enumerate(seqs):
        a[i, :len(s1)], b[i, :len(s2)], la[i], lb[i] = s1, s2, len(s1), len(s2)
        l1, l2 = [int(x) for x in s1], [int(x) for x in s2]
        s110[i] = ref.NeedlemanWunschAlignScore(l1, l2, -1, -1, 0, normalize=False)
        s231[i] = ref.NeedlemanWunschAlignScore(l1, l2, -2, -3, 1, normalize=False)
        per[i] = ref.get_seq_PER(l1, l2)
        assert per_oracle.align_score(l1, l2, -1, -1, 0) == s110[i] and per_oracle.align_score(l1, l2, -2, -3, 1) == s231[i]
        assert per_oracle.get_seq_PER(l1, l2) == per[i]
    assert per[-1] == 4. / 7.
    ARR.update(al_seq1=a, al_len1=la, al_seq2=b, al_len2=lb, al_score_110=s110, al_score_231=s231, al_per=per)


def main():
    search_cases()
    unit_cases()
    pairs()
    ARR["meta"] = np.array(json.dumps(META))
    path = os.path.join(OUT, "g26_per.npz")
    np.savez_compressed(path, **ARR)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
