"""float32 numpy statement of the reference's CTC prefix beam search (cpc/criterion/seq_alignment.py:11-61) on a trie, and its
alignment score (:89-117) in Python integers.  Used by tools/make_golden_per.py beside the reference (which it reproduces bit
for bit wherever no two candidates of a frame score the same) and by the tests as the statement the kernels are held to.

Prefixes are trie nodes (parent node, symbol) instead of the reference's comma-joined strings; the arithmetic is the reference's,
one numpy.float32 operation per operation of it.  Where scores are EQUAL the reference orders by the strings; this statement and
the kernel order by (rank of the extended prefix in the previous beam, symbol), a prefix that is not extended counting as its
own rank with symbol = blank.  `tie` tells whether any frame met equal scores among its first nKeep + 1 candidates: without one
the two orders cannot differ.
"""
import numpy as np

f32 = np.float32


def beam_search(probs, nKeep, blank):
    """-> ([(score float32, [labels]) best first], tie).  probs: [T, P] float32 probabilities."""
    p = np.asarray(probs, dtype=np.float32)
    T, P = p.shape
    if T == 0:
        raise ValueError("beam_search: no frame to decode (T = 0)")
    parent, sym, child = [-1], [-1], {}
    beam = [0]                                   # nodes, best first
    pb, pnb = {0: f32(1)}, {0: f32(0)}
    tie = False
    ranked = []
    for t in range(T):
        rank = {b: i for i, b in enumerate(beam)}
        cand = {}                                # node (or (parent, symbol) of a string without one) -> [pb, pnb, slot]
        for i, b in enumerate(beam):
            tot = f32(pb[b] + pnb[b])
            stay = f32(pnb[b] * p[t, sym[b]]) if b != 0 else f32(0)
            cand[b] = [f32(tot * p[t, blank]), stay, i * P + blank]
        for i, b in enumerate(beam):
            tot = f32(pb[b] + pnb[b])
            for c in range(P):
                if c == blank:
                    continue
                ext = f32((pb[b] if sym[b] == c else tot) * p[t, c])
                n = child.get((b, c))
                if n is not None and n in rank:  # the string is in the beam: one entry, as in the reference's dictionaries
                    cand[n][1] = f32(cand[n][1] + ext)
                else:
                    cand[(b, c) if n is None else n] = [f32(0), ext, i * P + c]
        ranked = sorted(((f32(v[0] + v[1]), v[2], k) for k, v in cand.items()), key=lambda x: (-x[0], x[1]))
        head = [x[0] for x in ranked[:nKeep + 1]]
        tie = tie or len(set(float(s) for s in head)) != len(head)
        beam, npb, npnb = [], {}, {}
        for score, _, k in ranked[:nKeep]:
            if isinstance(k, tuple):             # a survivor without a node yet
                child[k] = len(parent)
                parent.append(k[0])
                sym.append(k[1])
                n = child[k]
            else:
                n = k
            beam.append(n)
            npb[n], npnb[n] = cand[k][0], cand[k][1]
        pb, pnb = npb, npnb
    out = []
    for score, _, _ in ranked[:nKeep]:
        n = beam[len(out)]
        labels = []
        while n != 0:
            labels.append(sym[n])
            n = parent[n]
        out.append((score, labels[::-1]))
    return out, tie


def align_score(seq1, seq2, d, m, r):
    """-H[N1][N2] of the reference's NeedlemanWunschAlignScore before its normalisation: a Python integer."""
    n1, n2 = len(seq1), len(seq2)
    prev = [j * d for j in range(n2 + 1)]
    for i in range(n1):
        row = [(i + 1) * d] + [0] * n2
        for j in range(n2):
            match = r if int(seq1[i]) == int(seq2[j]) else m
            row[j + 1] = max(prev[j] + match, row[j] + d, prev[j + 1] + d)
        prev = row
    return -prev[n2]


def NeedlemanWunschAlignScore(seq1, seq2, d, m, r, normalize=True):
    res = align_score(seq1, seq2, d, m, r)
    if normalize:
        res /= float(len(seq1))
    return res


def get_seq_PER(seqLabels, detectedLabels):
    return NeedlemanWunschAlignScore(seqLabels, detectedLabels, -1, -1, 0, normalize=True)
