"""Pure-Python model of the X-drop extension of exact seeds, vmatch -l L
-hxdrop X | -exdrop X: a literal restatement of xdropseedextend
(Vmengine/xdropext.c:39-221), of evalhammingxdropleft / -right
(kurtz/xdrop.c:37-140) and of EVALXDROPEDIT (kurtz/xdrop.gen:2-201) with the
macros of kurtz/xdrop.c:151-261, on two Multiseqs given as lists of ints with
their separators.  Pinned to recorded runs of the reference by
scripts/make_golden_extend_xdrop.py and tests/test_extend_xdrop_host.py; the
engine is compared against it.

Two deliberately WRONG variants of the edit extension exist for one test
(frozen: a separator ends a slide but does not change ulen / vlen; unordered:
all diagonals of a generation slide under the lengths of its start): the
recorded behaviour depends on both."""
import numpy as np

from extend_model import MATCH_DTYPE, SEPARATOR, WILDCARD, multiseq

MATCHSCORE, MISMATCHSCORE, HALFMATCHSCORE = 2, -1, 1
DEFAULTSEEDLENGTH = 30
MAXDROP = 255


def seedlength_rule(S=0):
    """Vmatch/matchlenparm.c:40-46"""
    return int(S) if S else DEFAULTSEEDLENGTH


def cdiv(a, b):
    """C division: towards zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def evalhammingxdropright(useq, uoff, ulen, vseq, voff, vlen, X):
    """-> (ivalue, jvalue, score)"""
    bestend, total, best = -1, 0, 0
    t = 0
    while t < ulen and t < vlen:
        a = useq[uoff + t]
        if a == SEPARATOR:
            break
        b = vseq[voff + t]
        if b == SEPARATOR:
            break
        if a != b or a == WILDCARD:
            total += MISMATCHSCORE
        else:
            total += MATCHSCORE
        if total < best - X:
            break
        if best < total:
            best, bestend = total, t
        t += 1
    return bestend + 1, bestend + 1, best


def evalhammingxdropleft(useq, ulen, vseq, vlen, X, reachlength):
    """-> (ivalue, jvalue, score) or None: the seed is rejected"""
    bestend, matchlen, total, best = ulen, 0, 0, 0
    u, v = ulen - 1, vlen - 1
    while u >= 0 and v >= 0:
        a = useq[u]
        if a == SEPARATOR:
            break
        b = vseq[v]
        if b == SEPARATOR:
            break
        if a != b or a == WILDCARD:
            matchlen = 0
            total += MISMATCHSCORE
        else:
            matchlen += 1
            if matchlen >= reachlength:
                return None
            total += MATCHSCORE
        if total < best - X:
            break
        if best < total:
            best, bestend = total, u
        u -= 1
        v -= 1
    return ulen - bestend, ulen - bestend, best


class _Arrays:
    """useq, vseq with their lengths, which COMPARESYMBOLSSEP changes"""

    def __init__(self, left, useq, uoff, ulen, vseq, voff, vlen, frozen):
        self.left, self.frozen = left, frozen
        self.useq, self.uoff, self.ulen = useq, uoff, ulen
        self.vseq, self.voff, self.vlen = vseq, voff, vlen
        self.sepreads = 0      # left sides: separators read behind symbol 0

    def u(self, i):
        return self.useq[self.ulen - 1 - i] if self.left else \
            self.useq[self.uoff + i]

    def v(self, j):
        return self.vseq[self.vlen - 1 - j] if self.left else \
            self.vseq[self.voff + j]

    def compare(self, i, j, lengths=None):
        """COMPARESYMBOLSSEP: True the symbols match, False `break`;
        lengths: where the assignments go instead (the unordered variant)"""
        a = self.u(i)
        if a == SEPARATOR:
            self.sepreads += self.left and i > 0
            if lengths is not None:
                lengths.append(("u", i))
            elif not self.frozen:
                self.ulen = i
            return False
        b = self.v(j)
        if b == SEPARATOR:
            self.sepreads += self.left and j > 0
            if lengths is not None:
                lengths.append(("v", j))
            elif not self.frozen:
                self.vlen = j
            return False
        return not (a != b or a == WILDCARD)


def evalxdropedit(left, useq, uoff, ulen, vseq, voff, vlen, X, frozen=False,
                  unordered=False, trace=None, rows=None):
    """EVALXDROPEDITLEFT / -RIGHT -> (ivalue, jvalue, score).  left: uoff =
    voff = 0 and the symbols are useq[ulen - 1 - I].  trace: a dict that
    receives `generations`, `maxwidth` and `sepreads`; rows: a dict that
    receives, per generation, (smallest k, the rows with None for minus
    infinity, dmulti, the best score before it)"""
    s = _Arrays(left, useq, uoff, ulen, vseq, voff, vlen, frozen)
    dback = cdiv(-(X + HALFMATCHSCORE), MATCHSCORE - MISMATCHSCORE)
    dmulti = 0
    d, lower, upper = 1, 0, 0
    integermax = max(ulen, vlen)
    integermin = -integermax
    MINF = integermin
    i = 0
    while i < min(s.ulen, s.vlen):
        if not s.compare(i, i):
            break
        i += 1
    cur, cursmallest = [i], 0
    bestscore, bestivalue, bestjvalue = i + i, i, i
    ttab = [bestscore - X]
    maxwidth = 1
    if rows is not None:
        rows[0] = (0, [i], 0, None)
    while True:
        dmulti += MATCHSCORE - MISMATCHSCORE
        bestbefore = bestscore
        prev, prevsmallest = cur, cursmallest
        cur, cursmallest = [], lower - 1
        maxwidth = max(maxwidth, upper - lower + 3)
        at = lower - 1 - prevsmallest          # nextpreviousscore
        minisfinite = minisM = integermax
        maxisfinite = maxisN = integermin
        dbackvalue = -X if dback < 0 else ttab[dback]
        pending = [] if unordered else None
        for k in range(lower - 1, upper + 2):
            i = MINF
            if k < upper:                      # INSERTIONEOP
                tmp = prev[at + 1]
                if tmp != MINF and i < tmp:
                    i = tmp
            if lower <= k <= upper:            # MISMATCHEOP
                tmp = prev[at]
                if tmp != MINF and i <= tmp:
                    i = tmp + 1
            if lower < k:                      # DELETIONEOP
                tmp = prev[at - 1]
                if tmp != MINF and i <= tmp:
                    i = tmp + 1
            at += 1
            if i == MINF:
                cur.append(MINF)
                continue
            j = i - k
            if (i + j) * HALFMATCHSCORE - dmulti < dbackvalue:
                cur.append(MINF)
                continue
            while True:
                if i >= s.ulen:
                    break
                if j >= s.vlen:
                    break
                if not s.compare(i, j, pending):
                    break
                i += 1
                j += 1
            if j == s.vlen:
                maxisN = k
            if i == s.ulen and minisM > k:
                minisM = k
            if minisfinite > k:
                minisfinite = k
            maxisfinite = k
            cur.append(i)
            tmp = (i + j) * HALFMATCHSCORE - dmulti
            if bestscore < tmp:
                bestscore, bestivalue, bestjvalue = tmp, i, j
        if rows is not None:
            rows[d] = (cursmallest, [None if x == MINF else x for x in cur],
                       dmulti, bestbefore)
        for which, value in pending or ():
            if which == "u":
                s.ulen = value
            else:
                s.vlen = value
        lower = minisfinite if minisfinite > maxisN + 2 else maxisN + 2
        upper = maxisfinite if maxisfinite < minisM - 2 else minisM - 2
        if lower > upper + 2:
            break
        if maxisfinite < minisfinite:
            # no finite entry.  With integermax >= 2 the test above has said
            # so (lower = integermax, upper = -integermax); with arrays of
            # one symbol it reads 1 > 1 and the reference never returns:
            # the engine ends the side here, and so does the model
            assert integermax <= 1
            break
        ttab.append(bestscore - X)
        d += 1
        dback += 1
    if trace is not None:
        trace["generations"] = max(trace.get("generations", 0), d)
        trace["maxwidth"] = max(trace.get("maxwidth", 0), maxwidth)
        trace["sepreads"] = trace.get("sepreads", 0) + s.sepreads
    return bestivalue, bestjvalue, bestscore


def acceptmatch(length1, pos1, length2, pos2):
    if pos1 >= pos2:
        return False
    if pos1 + length1 - 1 < pos2:
        return True
    if pos1 + length1 >= pos2 + length2:
        return False
    return True


def score2distance(score, l1, l2):
    """EVALSCORE2DISTANCE, include/match.h:76-77"""
    return cdiv(l1 + l2 - score, 3) if score >= 0 else \
        -cdiv(l1 + l2 + score, 3)


def xdropseedextend(querycompare, xdropbelowscore, pos1, pos2, length, seq1,
                    seq2, seedlength, **variant):
    """rcmode or querycompare = querycompare, revmposorder = False ->
    (pos1, pos2, length1, length2, distance) or None"""
    n1, n2 = len(seq1), len(seq2)
    zero = (0, 0, 0)
    if xdropbelowscore < 0:
        left = evalhammingxdropleft(seq1, pos1, seq2, pos2, -xdropbelowscore,
                                    seedlength)
        if left is None:
            return None
        right = evalhammingxdropright(seq1, pos1 + length,
                                      n1 - (pos1 + length), seq2,
                                      pos2 + length, n2 - (pos2 + length),
                                      -xdropbelowscore)
    else:
        if pos1 == 0 or seq1[pos1 - 1] == SEPARATOR or pos2 == 0 or \
                seq2[pos2 - 1] == SEPARATOR:
            left = zero
        else:
            left = evalxdropedit(True, seq1, 0, pos1, seq2, 0, pos2,
                                 xdropbelowscore, **variant)
        if pos1 + length >= n1 or seq1[pos1 + length] == SEPARATOR or \
                pos2 + length >= n2 or seq2[pos2 + length] == SEPARATOR:
            right = zero
        else:
            right = evalxdropedit(False, seq1, pos1 + length,
                                  n1 - (pos1 + length), seq2, pos2 + length,
                                  n2 - (pos2 + length), xdropbelowscore,
                                  **variant)
    p1, p2 = pos1 - left[0], pos2 - left[1]
    exti, extj = left[0] + right[0], left[1] + right[1]
    if querycompare or p1 <= p2:
        length1, length2 = length + exti, length + extj
    else:
        p1, p2 = p2, p1
        length1, length2 = length + extj, length + exti
    if seq1[p1 + length1 - 1] == SEPARATOR:
        length1 -= 1
    if seq1[p1] == SEPARATOR:
        p1 += 1
        length1 -= 1
    if seq2[p2 + length2 - 1] == SEPARATOR:
        length2 -= 1
    if seq2[p2] == SEPARATOR:
        p2 += 1
        length2 -= 1
    if querycompare or acceptmatch(length1, p1, length2, p2):
        score = left[2] + right[2] + 2 * length
        if xdropbelowscore < 0:
            score = -score
        return p1, p2, length1, length2, score2distance(score, length1,
                                                        length2)
    return None


def pack(length1, length2, start, distance):
    return (length1 | length2 << 32, start | abs(distance) << 32)


def matches(seeds, text, X, hamming, S=0, queries=None, **variant):
    """what xdropseedextend gives for every seed: [(pos1, pos2 in the second
    Multiseq, length1, length2, distance) or None], and where the sequences
    of the batch begin in that Multiseq"""
    assert 1 <= X <= MAXDROP
    seedlength = seedlength_rule(S)
    seq1 = [int(c) for c in text]
    if queries is None:
        seq2, qstart = seq1, None
    else:
        seq2, qstart = multiseq(*queries)
    out = []
    for m in seeds:
        length, pos1 = int(m["length"]), int(m["dbstart"])
        if queries is None:
            pos2 = int(m["queryseq"])
        else:
            pos2 = qstart[int(m["queryseq"])] + int(m["querystart"])
        out.append(xdropseedextend(queries is not None,
                                   -X if hamming else X, pos1, pos2, length,
                                   seq1, seq2, seedlength, **variant))
    return out, qstart


def extend(seeds, text, L, X, hamming, S=0, queries=None, **variant):
    """seeds: MATCH_DTYPE records of the MEM search (queries = (symbols,
    start, length) of the batch they refer to) or of the repeat search
    (queries None) -> the records of the matches with both lengths >= L
    (matchokay, Vmatch/mokay.c:16-24), in the order of their seeds"""
    found, qstart = matches(seeds, text, X, hamming, S, queries, **variant)
    out = []
    for m, e in zip(seeds, found):
        if e is None:
            continue
        p1, p2, length1, length2, distance = e
        if length1 < L or length2 < L:
            continue
        if queries is None:
            lf, sf = pack(length1, length2, 0, distance)
            out.append((lf, p1, p2, sf))
        else:
            pos2 = qstart[int(m["queryseq"])] + int(m["querystart"])
            lf, sf = pack(length1, length2,
                          int(m["querystart"]) - (pos2 - p2), distance)
            out.append((lf, p1, int(m["queryseq"]), sf))
    res = np.zeros(len(out), MATCH_DTYPE)
    for i, o in enumerate(out):
        res[i] = o
    return res


def lengths1(rec):
    return rec["length"] & np.uint64(0xFFFFFFFF)


def lengths2(rec):
    return rec["length"] >> np.uint64(32)


def starts(rec):
    return rec["querystart"] & np.uint64(0xFFFFFFFF)


def distances(rec):
    return rec["querystart"] >> np.uint64(32)
