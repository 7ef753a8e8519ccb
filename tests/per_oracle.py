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


def _key(score):
    """The kernel's select key of a score: 1 + its f32 bit pattern (0 is kept for a slot without a candidate)."""
    u = int(f32(score).view(np.uint32))
    return u if u == 0xffffffff else u + 1


def beam_search(probs, nKeep, blank, stats=None):
    """-> ([(score float32, [labels]) best first], tie).  probs: [T, P] float32 probabilities.

    stats: a dict that is filled with what the input made the search do (the result does not depend on it):
      levels     one entry per frame with more candidates than nKeep: the most significant byte (3..0) in which the keys
                 (1 + f32 bits) of the nKeep-th and the (nKeep + 1)-th ranked candidate differ -- the byte at which a radix select,
                 most significant byte first, can stop -- or "tie" when the two are equal
      groups     one dict per "tie" frame: frame, size (candidates that carry the cut score), lo / hi (their smallest and largest
                 slot), need (how many of them the beam takes) and taken_hi (the slot of the last one taken, in slot order)
      folds      extensions whose string already was in the beam (added to that entry)
      reentries  survivors that had a node and were not in the previous frame's beam
      rejoined   those of them that met a child of theirs in that beam: from then on the child's entry takes the extension of
                 its parent again, which needs the survivor to be the node it was
      max_beam   the largest beam that a frame extended (nKeep: some frame used all nKeep * P slots)
      nodes      nodes of the trie at the end, the root included"""
    if stats is not None:
        stats.update(levels=[], groups=[], folds=0, reentries=0, rejoined=0, max_beam=0, nodes=1)
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
                    if stats is not None:
                        stats["folds"] += 1
                else:
                    cand[(b, c) if n is None else n] = [f32(0), ext, i * P + c]
        ranked = sorted(((f32(v[0] + v[1]), v[2], k) for k, v in cand.items()), key=lambda x: (-x[0], x[1]))
        head = [x[0] for x in ranked[:nKeep + 1]]
        tie = tie or len(set(float(s) for s in head)) != len(head)
        if stats is not None:
            _record(stats, t, ranked, nKeep, rank, parent)
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
    if stats is not None:
        stats["nodes"] = len(parent)
    return out, tie


def _record(stats, t, ranked, nKeep, rank, parent):
    """One frame's entries of beam_search's stats: ranked = [(score, slot, node or (parent, symbol))] best first, rank = the
    beam that the frame extended, parent = the trie's parent of every node."""
    stats["max_beam"] = max(stats["max_beam"], len(rank))
    back = [k for _, _, k in ranked[:nKeep] if not isinstance(k, tuple) and k not in rank]
    stats["reentries"] += len(back)
    stats["rejoined"] += sum(1 for k in back if any(parent[b] == k for b in rank))
    if len(ranked) <= nKeep:
        return
    last, following = _key(ranked[nKeep - 1][0]), _key(ranked[nKeep][0])
    if last != following:
        stats["levels"].append(((last ^ following).bit_length() - 1) // 8)
        return
    stats["levels"].append("tie")
    slots = sorted(slot for score, slot, _ in ranked if _key(score) == last)
    need = sum(1 for score, _, _ in ranked[:nKeep] if _key(score) == last)
    stats["groups"].append(dict(frame=t, size=len(slots), lo=slots[0], hi=slots[-1], need=need, taken_hi=slots[need - 1]))


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
