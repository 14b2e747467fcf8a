"""Pure-Python model of the Hamming extension of exact seeds, vmatch -l L -h K
outside -complete: a direct restatement of hammingextend
(kurtz/extendHD.c:56-374) with cmpmatches (include/extcmp.c) and the
E-value table of kurtz/evalues.c:307-386, on two Multiseqs given as byte
arrays with their separators.  Pinned to recorded runs of the reference by
scripts/make_golden_extend.py and tests/test_extend_host.py; the engine is
compared against it."""
import numpy as np

SEPARATOR = 255
WILDCARD = 254
LENGTHBITS = 48

MATCH_DTYPE = np.dtype([("length", "<u8"), ("dbstart", "<u8"),
                        ("queryseq", "<u8"), ("querystart", "<u8")])


def seedlength_rule(L, K, S=0):
    """Vmatch/matchlenparm.c:11-22"""
    return max(int(S), int(L) // (int(K) + 1))


class Evalues:
    """inithammingEvalues / incprecomputehammingEvalues / inclookupEvalue"""

    SMALLEST = 1e-300  # SMALLESTEVALUE, kurtz/evalues.c

    def __init__(self, numofchars):
        self.p = 1.0 / numofchars
        self.first = self.p * ((1.0 - self.p) * (1.0 - self.p))
        self.lines = []

    def line(self, k):
        while len(self.lines) <= k:
            kk = len(self.lines)
            prob = self.first
            self.first *= ((float(kk + 2) / (kk + 1)) * (1.0 - self.p))
            row, l = [], kk + 1
            while prob > self.SMALLEST:
                row.append(prob)
                prob *= ((l + 1) * self.p / (l + 1 - kk))
                l += 1
            self.lines.append(row)
        return self.lines[k]

    def lookup(self, distance, length):
        """the value for `distance` mismatches in `length` symbols; a length
        the line does not hold reads 0.0"""
        row = self.line(distance)
        i = length - (distance + 1)
        return row[i] if 0 <= i < len(row) else 0.0


def cmpmatches(ev, dist1, dist2, len1, len2):
    e1, e2 = 1.0 * ev.lookup(dist1, len1), 1.0 * ev.lookup(dist2, len2)
    if e1 < e2:
        return -1
    if e1 > e2:
        return 1
    id1 = 100.0 * (1.0 - float(dist1) / len1)
    id2 = 100.0 * (1.0 - float(dist2) / len2)
    if id1 < id2:
        return 1
    if id1 > id2:
        return -1
    if len1 < len2:
        return 1
    if len1 > len2:
        return -1
    return 1


def _left(look, maxdist, searchlength, seq1, r1, seq2, r2):
    for h in range(maxdist + 1):
        look[h] = 0
    h, i1, i2 = 1, r1, r2
    while True:
        a, b = seq1[i1], seq2[i2]
        if a == SEPARATOR or b == SEPARATOR:
            look[h] = r1 - i1 + 1
            break
        if a != b or a == WILDCARD:
            look[h] = r1 - i1 + 1
            if h == maxdist or look[h] - look[h - 1] > searchlength:
                break
            h += 1
        if i1 == 0 or i2 == 0:
            look[h] = r1 - i1 + 2
            break
        i1 -= 1
        i2 -= 1
    if look[h] - look[h - 1] > searchlength:
        return h - 1
    return h


def _right(look, maxdist, seq1, last1, l1, seq2, last2, l2):
    for h in range(maxdist + 1):
        look[h] = 0
    h, i1, i2 = 1, l1, l2
    while True:
        a, b = seq1[i1], seq2[i2]
        if a == SEPARATOR or b == SEPARATOR:
            look[h] = i1 - l1 + 1
            break
        if a != b or a == WILDCARD:
            look[h] = i1 - l1 + 1
            if h == maxdist:
                break
            h += 1
        if i1 == last1 or i2 == last2:
            look[h] = i1 - l1 + 2
            break
        i1 += 1
        i2 += 1
    return h


def hammingextend(ev, maxdist, leastlength, seedlength, pos1, pos2, length,
                  seq1, seq2):
    """-> (shift to the left, length, distance) or None; seq1, seq2: lists of
    ints, the two Multiseqs"""
    n1, n2 = len(seq1), len(seq2)
    size = max(maxdist + 1, 3)
    ll, lr = [0] * size, [0] * size
    if pos1 > 1 and pos2 > 1:
        if seq1[pos1 - 1] == SEPARATOR or seq2[pos2 - 1] == SEPARATOR:
            hleft = 0
        else:
            hleft = _left(ll, maxdist, seedlength, seq1, pos1 - 2, seq2,
                          pos2 - 2)
    elif (pos1 == 0 or pos2 == 0 or seq1[pos1 - 1] == SEPARATOR or
          seq2[pos2 - 1] == SEPARATOR):
        hleft = 0
    else:
        hleft, ll[0], ll[1] = 1, 0, 1
    r1, r2 = pos1 + length, pos2 + length
    if r1 < n1 - 1 and r2 < n2 - 1:
        if seq1[r1] == SEPARATOR or seq2[r2] == SEPARATOR:
            hright = 0
        else:
            hright = _right(lr, maxdist, seq1, n1 - 1, r1 + 1, seq2, n2 - 1,
                            r2 + 1)
    elif (r1 >= n1 or r2 >= n2 or seq1[r1] == SEPARATOR or
          seq2[r2] == SEPARATOR):
        hright = 0
    else:
        hright, lr[0], lr[1] = 1, 0, 1
    remain = 0 if length >= leastlength else leastlength - length
    if ll[hleft] + lr[hright] < remain:
        return None
    if hleft + hright < maxdist:
        maxdist = hleft + hright
    best = None
    for dist in range(maxdist + 1):
        lookindex = 0 if dist < hright else dist - hright
        while lookindex <= min(dist, hleft):
            left = ll[lookindex]
            ext = left + lr[dist - lookindex]
            if ext >= remain:
                if best is None or cmpmatches(ev, best[2], dist, best[1],
                                              length + ext) == 1:
                    best = (left, length + ext, dist)
            lookindex += 1
    return best


def multiseq(symbols, start, length):
    """the reference's Multiseq of the sequences symbols[start[i] : start[i] +
    length[i]]: separators between them -> (list of ints, start of each)"""
    out, starts = [], []
    for i, (s, l) in enumerate(zip(start, length)):
        if i:
            out.append(SEPARATOR)
        starts.append(len(out))
        out.extend(int(c) for c in symbols[int(s):int(s) + int(l)])
    return out, starts


def extend(seeds, text, numofchars, L, K, S=0, queries=None, evalues=None):
    """seeds: MATCH_DTYPE records of the MEM search (queries = (symbols,
    start, length) of the batch they refer to) or of the repeat search
    (queries None) -> the records of the matches, in the order of their
    seeds, the distance in the top 16 bits of the length"""
    ev = evalues or Evalues(numofchars)
    seedlength = seedlength_rule(L, K, S)
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
        best = hammingextend(ev, K, L, seedlength, pos1, pos2, length, seq1,
                             seq2)
        if best is None:
            continue
        shift, newlen, dist = best
        if queries is None:
            out.append((newlen | dist << LENGTHBITS, pos1 - shift,
                        pos2 - shift, 0))
        else:
            out.append((newlen | dist << LENGTHBITS, pos1 - shift,
                        int(m["queryseq"]), int(m["querystart"]) - shift))
    res = np.zeros(len(out), MATCH_DTYPE)
    for i, o in enumerate(out):
        res[i] = o
    return res


def lengths(rec):
    return rec["length"] & np.uint64((1 << LENGTHBITS) - 1)


def distances(rec):
    return rec["length"] >> np.uint64(LENGTHBITS)
