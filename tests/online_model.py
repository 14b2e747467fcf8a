"""A literal Python model of vmatch -online -complete: one function per
function of the reference, separate from the rules the library states in
online_rules.h.  Symbols are the mapped ones (0 .. numofchars - 1, WILDCARD,
SEPARATOR); a text is a bytes object or a uint8 array.  Python integers stand
for the DPbitvector4 / DPbitvector8 words: the bits from m on are masked away,
which changes no bit below m.

    findexactcompletematchesonline    Vmengine/exactcompl.c:277-325
    hammingcompletematchesonline      Vmengine/hamcompl.c:9-56
    getEqs / getEqsrev                kurtz-basic/getEqs.gen
    CheckMatchPosition                CHECKMATCHPOSITION, edistcompl.c:33-80
    edistmyersbitvectorAPM            edistcompl.c:261-384 (APM4 and APM8)
    edistukkonencutoff                edistcompl.c:82-172
    shortpatternlongestmatch          longestmatch.c:85-153 (short and medium)
    longpatternlongestmatch           longestmatch.c:18-71
    edistprocessstartpos              approxcompl.c:14-65
    findedistcompletematchesonline    edistcompl.c:458-513
    findcompletematches               fcomplete.c:209-261 over all queries
"""
import functools

import numpy as np

SEPARATOR = 255
WILDCARD = 254
MATCH_DTYPE = np.dtype([("length", "<u8"), ("dbstart", "<u8"),
                        ("queryseq", "<u8"), ("querystart", "<u8")])


def isspecial(c):
    return c >= WILDCARD


def findexactcompletematchesonline(seq, pattern, process):
    plen, n = len(pattern), len(seq)
    if not (0 < plen <= n):
        return
    rmostocc = [plen] * 256
    for ppos in range(plen - 1):
        if not isspecial(pattern[ppos]):
            rmostocc[pattern[ppos]] = plen - ppos - 1
    s = 0
    while s <= n - plen:
        i = plen - 1
        while not isspecial(seq[s + i]) and pattern[i] == seq[s + i]:
            if i == 0:
                process(plen, s, 0)
                break
            i -= 1
        s += rmostocc[seq[s + plen - 1]]


def hammingcompletematchesonline(seq, pattern, threshold, process):
    plen = len(pattern)
    p = len(seq) - plen
    while p >= 0:
        if seq[p] == SEPARATOR:
            p -= plen
            continue
        countmm, skip = 0, False
        for s in range(plen):
            if seq[p + s] == SEPARATOR:
                skip = True
                break
            if seq[p + s] != pattern[s]:
                countmm += 1
                if countmm > threshold:
                    break
        if not skip and countmm <= threshold:
            process(plen, p, -countmm)
        p -= 1


def getEqs(u):
    eqs = [0] * 256
    for i, c in enumerate(u):
        assert c != SEPARATOR
        if c != WILDCARD:
            eqs[c] |= 1 << i
    return eqs


def getEqsrev(u):
    return getEqs(u[::-1])


def shortpatternlongestmatch(eqs, ulen, v):
    """-> (length, distance); v is the text from the start position on, cut
    to maxlength"""
    mask = (1 << ulen) - 1
    pv, mv, ebit, score = mask, 0, 1 << (ulen - 1), ulen
    longest = (0, ulen)
    for j, c in enumerate(v):
        if c == SEPARATOR:
            return longest
        eq = eqs[c]
        xv = eq | mv
        xh = ((((eq & pv) + pv) ^ pv) | eq) & mask
        ph = (mv | ~(xh | pv)) & mask
        mh = pv & xh
        if ph & ebit:
            score += 1
        elif mh & ebit:
            score -= 1
        ph = ((ph << 1) | 1) & mask
        pv = ((mh << 1) | ~(xv | ph)) & mask
        mv = ph & xv
        if longest[1] >= score:
            longest = (j + 1, score)
    return longest


def longpatternlongestmatch(u, v):
    """the column of the reference, a whole column per numpy operation:
    ecol[i] = min(ecol[i - 1] + 1, nw + (u[i - 1] differs), we + 1), the
    first term as a running minimum"""
    ulen = len(u)
    u = np.frombuffer(bytes(bytearray(u)), np.uint8)
    idx = np.arange(ulen + 1, dtype=np.int64)
    ecol = idx.copy()
    longest = (0, ulen)
    for j, c in enumerate(v):
        if c == SEPARATOR:
            return longest
        differs = ((u != c) | (u == WILDCARD)).astype(np.int64)
        full = np.concatenate(([ecol[0] + 1],
                               np.minimum(ecol[:-1] + differs, ecol[1:] + 1)))
        ecol = np.minimum.accumulate(full - idx) + idx
        if longest[1] >= ecol[ulen]:
            longest = (j + 1, int(ecol[ulen]))
    return longest


@functools.lru_cache(maxsize=1 << 14)
def _longestmatch(pattern, v):
    """(what the two functions return depends on their arguments alone: in a
    text of low complexity the same stretch comes up thousands of times)"""
    if len(pattern) > 64:
        return longpatternlongestmatch(pattern, v)
    return shortpatternlongestmatch(getEqs(pattern), len(pattern), v)


def edistprocessstartpos(seq, pattern, startpos, maxlength, process):
    v = seq[startpos:startpos + maxlength]
    if isinstance(seq, bytes) and isinstance(pattern, bytes):
        longest = _longestmatch(pattern, v)
    elif len(pattern) > 64:
        longest = longpatternlongestmatch(pattern, v)
    else:
        longest = shortpatternlongestmatch(getEqs(pattern), len(pattern), v)
    process(longest[0], startpos, longest[1])


class CheckMatchPosition:
    """the state a scan carries from start position to start position"""

    def __init__(self, seq, pattern, threshold, removeredundant, process):
        self.seq, self.pattern, self.process = seq, pattern, process
        self.plenplusthreshold = len(pattern) + threshold
        self.removeredundant = removeredundant
        self.foundmatch, self.relpos1, self.distance = False, 0, 0
        self.dropped = 0   # hits that changed nothing (remred)

    def setmaxlength(self, pos):
        return min(len(self.seq) - pos, self.plenplusthreshold)

    def flush(self):
        edistprocessstartpos(self.seq, self.pattern, self.relpos1,
                             self.setmaxlength(self.relpos1), self.process)

    def __call__(self, currentpos1, score):
        if not self.removeredundant:
            edistprocessstartpos(self.seq, self.pattern, currentpos1,
                                 self.setmaxlength(currentpos1), self.process)
            return
        if self.foundmatch:
            if self.relpos1 == currentpos1 + 1:
                if score < self.distance:
                    self.relpos1, self.distance = currentpos1, score
                else:
                    self.dropped += 1
            else:
                self.flush()
                self.relpos1, self.distance = currentpos1, score
        else:
            self.relpos1, self.distance = currentpos1, score
            self.foundmatch = True

    def end(self):
        if self.removeredundant and self.foundmatch:
            self.flush()


def edistmyersbitvectorAPM(seq, pattern, threshold, check):
    plen = len(pattern)
    eqsrev = getEqsrev(pattern)
    mask = (1 << plen) - 1
    pv, mv, ebit, score = mask, 0, 1 << (plen - 1), plen
    for p in range(len(seq) - 1, -1, -1):
        c = seq[p]
        if c == SEPARATOR:
            pv, mv, score = mask, 0, plen
            continue
        eq = eqsrev[c]
        xv = eq | mv
        xh = ((((eq & pv) + pv) ^ pv) | eq) & mask
        ph = (mv | ~(xh | pv)) & mask
        mh = pv & xh
        if ph & ebit:
            score += 1
        elif mh & ebit:
            score -= 1
        ph = (ph << 1) & mask
        pv = ((mh << 1) | ~(xv | ph)) & mask
        mv = ph & xv
        if score <= threshold:
            check(p, score)
    check.end()


def edistukkonencutoff(seq, pattern, threshold, check):
    plen = len(pattern)
    dcol = [0] * (plen + 2)
    for i in range(threshold + 1):
        if i <= plen + 1:
            dcol[i] = i
    end = threshold + 1
    for p in range(len(seq) - 1, -1, -1):
        c = seq[p]
        if c == SEPARATOR:
            end = threshold + 1
            for i in range(threshold + 1):
                dcol[i] = i
            continue
        nw, d, pp = 0, 1, plen - 1
        while d < end:
            we = dcol[d]
            if c == pattern[pp]:
                dcol[d] = nw
            elif dcol[d - 1] < nw:
                dcol[d] = dcol[d - 1] + 1
            elif we < nw:
                dcol[d] += 1
            else:
                dcol[d] = nw + 1
            nw = we
            d += 1
            pp -= 1
        if pp >= 0 and (c == pattern[pp] or threshold > dcol[end - 1]):
            dcol[d] = threshold
            end += 1
        else:
            d = end - 1
            while dcol[d] > threshold:
                d -= 1
            end = d + 1
        if end == plen + 1:
            check(p, dcol[end - 1])
    check.end()


def findedistcompletematchesonline(seq, pattern, threshold, removeredundant,
                                   process):
    check = CheckMatchPosition(seq, pattern, threshold, removeredundant,
                               process)
    if len(pattern) > 64:
        assert threshold < len(pattern), "dcol of the reference would overflow"
        edistukkonencutoff(seq, pattern, threshold, check)
    else:
        edistmyersbitvectorAPM(seq, pattern, threshold, check)
    return check


EXACT, EDIST, HAMMING = 0, 1, 2


def threshold_of(plen, distvalue, percent):
    return plen * distvalue // 100 if percent else distvalue


def query_matches(seq, pattern, mode, distvalue=0, percent=False,
                  removeredundant=False, info=None):
    """[(length1, position1, distance as the reference stores it)] of one
    query; info: a dict that receives what the scan saw"""
    out = []

    def process(length, pos, distance):
        out.append((length, pos, distance))
    seq = bytes(bytearray(seq))
    pattern = bytes(bytearray(pattern))
    if len(pattern) == 0:
        return out
    k = threshold_of(len(pattern), distvalue, percent)
    if mode == EXACT:
        findexactcompletematchesonline(seq, pattern, process)
    elif mode == HAMMING:
        hammingcompletematchesonline(seq, pattern, k, process)
    else:
        check = findedistcompletematchesonline(seq, pattern, k,
                                               removeredundant, process)
        if info is not None:
            info["dropped"] = info.get("dropped", 0) + check.dropped
    return out


def findcompletematches(seq, queries, mode, distvalue=0, percent=False,
                        removeredundant=False, offset=0, info=None):
    """queries: a list of symbol arrays -> the records of the engine, in the
    order of the reference (the distance of -h as the number of mismatches)"""
    rows = []
    for i, q in enumerate(queries):
        for length, pos, dist in query_matches(seq, q, mode, distvalue,
                                               percent, removeredundant, info):
            rows.append((length, pos, i + offset, abs(dist)))
    return np.array(rows, MATCH_DTYPE).reshape(-1)
