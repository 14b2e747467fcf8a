"""The repeat family from its definitions: no suffix array, no lcp table.

Positions are text positions; a symbol is regular below the wildcard code,
special otherwise.  lce(i, j) is the number of regular symbols the suffixes
at i and j share before they differ, meet a special symbol or the end of the
text.

  maximal repeat       a pair i < j with d = lce(i, j) >= L that cannot be
                       extended to the left: i = 0, or the characters in front
                       differ, or one of them is special
  supermaximal repeat  the full occurrence set of a string of d >= L symbols,
                       when every two of its occurrences extend by exactly d
                       and the regular characters in front of them are
                       pairwise different: all pairs of the set
  tandem               t[v:v+d] == t[v+d:v+2d], d >= L, the unit followed by
                       at least two different continuations among its
                       occurrences (a special symbol or the end of the text is
                       a continuation of its own); reported unless t[v] ==
                       t[v+2d] with both regular -- a repeat that ends with
                       the text is always reported
  index with queries   only pairs with i below and j above the separating
                       position

Every function returns a set of (length, start1, start2).  Start positions
are grouped by their L-gram first, so that only positions that can pair are
compared; within a group all pairs are looked at, which is what keeps the
model to small groups (see repeat_cases.MODELLED)."""
import numpy as np

import helpers as H


class Text:
    def __init__(self, tis):
        self.t = np.ascontiguousarray(tis, np.uint8)
        self.n = len(self.t)
        self.bytes = self.t.tobytes()
        special = np.flatnonzero(self.t >= H.WILDCARD)
        # end of the run of regular symbols that starts at p
        self.runend = np.full(self.n + 1, self.n, np.int64)
        if len(special):
            nxt = np.searchsorted(special, np.arange(self.n))
            have = nxt < len(special)
            self.runend[:self.n][have] = special[nxt[have]]

    def run(self, p):
        return self.bytes[p:int(self.runend[p])]

    def left(self, p):
        """the character in front of p; None: not a regular symbol"""
        if p == 0 or self.t[p - 1] >= H.WILDCARD:
            return None
        return int(self.t[p - 1])

    def groups(self, L):
        """start positions by the L regular symbols that follow them"""
        g = {}
        for p in range(self.n):
            if self.runend[p] - p >= L:
                g.setdefault(self.bytes[p:p + L], []).append(p)
        return [v for v in g.values() if len(v) > 1]


def common(a, b):
    """length of the common prefix of two byte strings"""
    lo, hi = 0, min(len(a), len(b))
    if a[:hi] == b[:hi]:
        return hi
    while lo + 1 < hi:               # a[:lo] == b[:lo], a[:hi] != b[:hi]
        mid = (lo + hi) // 2
        if a[lo:mid] == b[lo:mid]:
            lo = mid
        else:
            hi = mid
    return lo


def maximal_repeats(tis, L, querysep=None):
    x, out = Text(tis), set()
    for g in x.groups(L):
        runs = [x.run(p) for p in g]
        lefts = [x.left(p) for p in g]
        for a in range(len(g)):
            for b in range(a + 1, len(g)):
                if (lefts[a] is not None and lefts[a] == lefts[b]):
                    continue
                i, j = g[a], g[b]
                if querysep is not None and not i < querysep < j:
                    continue
                out.add((common(runs[a], runs[b]), i, j))
    return out


def supermaximal_repeats(tis, L):
    x, out = Text(tis), set()
    for g in x.groups(L):
        runs = [x.run(p) for p in g]
        k = len(g)
        lce = np.zeros((k, k), np.int64)
        for a in range(k):
            for b in range(a + 1, k):
                lce[a, b] = lce[b, a] = common(runs[a], runs[b])
        done = set()
        for a in range(k):
            for d in set(int(v) for v in lce[a] if v >= L):
                # the occurrences of the d symbols at g[a]
                occ = tuple(b for b in range(k) if b == a or lce[a, b] >= d)
                if (occ, d) in done:
                    continue
                done.add((occ, d))
                sub = lce[np.ix_(occ, occ)]
                exact = all(sub[r, s] == d for r in range(len(occ))
                            for s in range(len(occ)) if r != s)
                lefts = [x.left(g[b]) for b in occ]
                lefts = [c for c in lefts if c is not None]
                if exact and len(lefts) == len(set(lefts)):
                    for r in range(len(occ)):
                        for s in range(r + 1, len(occ)):
                            out.add((d, g[occ[r]], g[occ[s]]))
    return out


def tandems(tis, L):
    x, out = Text(tis), set()
    t, n = x.t, x.n
    regular = t < H.WILDCARD
    for d in range(L, n // 2 + 1):
        same = (t[:n - d] == t[d:]) & regular[:n - d]
        if same.sum() < d:
            continue
        # v with same[v .. v+d-1]: running count of equal symbols
        c = np.concatenate(([0], np.cumsum(same)))
        full = np.flatnonzero(c[d:] - c[:len(c) - d] == d)
        branching = {}
        for v in (int(v) for v in full):
            unit = x.bytes[v:v + d]
            if unit not in branching:
                nexts, regs, p = 0, set(), x.bytes.find(unit)
                while p >= 0:
                    if p + d < n and regular[p + d]:
                        regs.add(x.bytes[p + d])
                    else:
                        nexts += 1
                    p = x.bytes.find(unit, p + 1)
                branching[unit] = nexts + len(regs) >= 2
            if not branching[unit]:
                continue
            if v + 2 * d < n and t[v] == t[v + 2 * d] and regular[v]:
                continue
            out.add((d, v, v + d))
    return out


MODELS = {"repeats": maximal_repeats, "supermax": supermaximal_repeats,
          "tandem": tandems}


def as_set(m):
    """an oracle or product list -> the model's set"""
    return set(zip((int(v) for v in m["length"]),
                   (int(v) for v in m["dbstart"]),
                   (int(v) for v in m["queryseq"])))
