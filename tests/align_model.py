"""A literal Python restatement of what vmatch -s does with one match: the
edit script (greedyedistalign with backtracefront, kurtz/galign.c:215-420 on
kurtz/front.gen; hammingalignment, galign.c:158-213; alignequalstrings,
galign.c:135-156) and the text showalignment prints for it
(kurtz/showalign.c: fillthelines 664-862, showeditopline 1706-1812,
formatalignment 1886-2048).  Slow and plain: the reference's loops, one symbol
at a time.  scripts/make_golden_align.py pins it to the output of the real
vmatch; the host and the device code are tested against it."""
import numpy as np

WILDCARD, SEPARATOR = 254, 255
MAXIDENTICALLENGTH = 16383            # include/alignment.h:43-46
DELETIONEOP, INSERTIONEOP, MISMATCHEOP = 1 << 14, 1 << 15, 3 << 14
GAP = SEPARATOR - 3                   # ABSTRACTGAPSYMBOL, alignment.h:154
NUMWIDTH = 12                         # showalign.c:600
REPLACEMENT, INSERTION, DELETION = 1, 2, 3


def symequal(a, b):
    """COMPARESYMBOLS: a special symbol equals nothing"""
    return a == b and a < WILDCARD


def add_identical(out, lenid):
    """ADDIDENTICAL, galign.c:78-89 -- literally: the first piece is
    lenid & 16383, not lenid % 16383"""
    while True:
        out.append(lenid & MAXIDENTICALLENGTH)
        if lenid <= MAXIDENTICALLENGTH:
            break
        lenid -= MAXIDENTICALLENGTH


def equal_script(length):
    out = []
    add_identical(out, length)
    return out


def hamming_script(u, v):
    """back to front; a position with a != b or a special a is a mismatch"""
    out, lenid, inrange = [], 0, False
    for i in range(len(u) - 1, -1, -1):
        a, b = int(u[i]), int(v[i])
        if a != b or a >= WILDCARD:
            if inrange:
                add_identical(out, lenid)
                inrange = False
            out.append(MISMATCHEOP)
        elif inrange:
            lenid += 1
        else:
            lenid, inrange = 1, True
    if inrange:
        add_identical(out, lenid)
    return out


class Fronts:
    """what greedyedistalign leaves behind: the real distance, the direction
    of every entry, the row every slide began and ended at"""

    def __init__(self):
        self.distance = None
        self.direction = {}      # (generation, diagonal) -> 1, 2, 3
        self.begin = {}          # ... -> the row the forward slide began at
        self.row = {}            # ... -> the stored row (None: minus infinity)


def fronts(u, v, maxdist, sametext=None):
    """greedyedistalign up to the backtrace.  sametext: None, or pv - pu of
    two substrings of ONE array (front.gen:120: uptr == vptr).  -> Fronts, or
    None if the distance is above maxdist (the reference's error)"""
    ulen, vlen = len(u), len(v)
    neg = -(1 << 40)
    f = Fronts()

    def slide(t, k):
        while t < ulen and t + k < vlen and symequal(int(u[t]), int(v[t + k])):
            t += 1
        return t

    prev = {0: slide(0, 0) if ulen and vlen else 0}
    f.row[(0, 0)] = prev[0]
    f.begin[(0, 0)] = 0
    if ulen == vlen and prev[0] == vlen:
        f.distance = 0
        return f
    for p in range(1, maxdist + 1):
        # (the narrower fronts of generations above min(ulen, vlen) are not
        # restated: a record whose distance is above a length is refused)
        assert p <= min(ulen, vlen)
        cur = {}
        for k in range(-p, p + 1):
            t = prev.get(k, neg) + 1
            direction = REPLACEMENT
            value = prev.get(k - 1, neg)
            if t < value:
                t, direction = value, INSERTION
            value = prev.get(k + 1, neg) + 1
            if t < value:
                t, direction = value, DELETION
            f.direction[(p, k)] = direction
            if t < 0 or t + k < 0:
                cur[k] = neg
                continue
            f.begin[(p, k)] = t
            if ulen != 0 and vlen != 0:
                if sametext is not None and t == sametext + t + k:
                    t = ulen - 1
                else:
                    t = slide(t, k)
            cur[k] = neg if (t > ulen or t + k > vlen) else t
            if cur[k] != neg:
                f.row[(p, k)] = cur[k]
        prev = cur
        if prev.get(vlen - ulen, neg) == ulen:
            f.distance = p
            return f
    return None


def backtrace(f, u, v):
    """backtracefront -> (script, overshoot): overshoot = a backward slide
    went below the row its forward slide began at"""
    ulen, vlen = len(u), len(v)
    out, overshoot = [], False
    d, i, j = vlen - ulen, ulen - 1, vlen - 1
    for k in range(f.distance, 0, -1):
        starti = i
        while i >= 0 and j >= 0 and symequal(int(u[i]), int(v[j])):
            i -= 1
            j -= 1
        if i < starti:
            add_identical(out, starti - i)
        if (k, d) in f.begin and i + 1 < f.begin[(k, d)]:
            overshoot = True
        direction = f.direction[(k, d)]
        if direction == REPLACEMENT:
            out.append(MISMATCHEOP)
            i -= 1
            j -= 1
        elif direction == DELETION:
            out.append(DELETIONEOP)
            i -= 1
            d += 1
        else:
            out.append(INSERTIONEOP)
            j -= 1
            d -= 1
    if i >= 0:
        add_identical(out, i + 1)
    return out, overshoot


def edist_script(u, v, maxdist, sametext=None):
    """-> (script, real distance, overshoot) or None (distance > maxdist)"""
    f = fronts(u, v, maxdist, sametext)
    if f is None:
        return None
    script, overshoot = backtrace(f, u, v)
    return script, f.distance, overshoot


def script(u, v, distance, sametext=None):
    """shownormalstringout, echomatch.c:587-658; distance: the stored one,
    negative for a Hamming match"""
    if distance == 0:
        return equal_script(len(u))
    if distance < 0:
        return hamming_script(u, v)
    got = edist_script(u, v, distance, sametext)
    return None if got is None else got[0]


def consumed(words):
    """symbols of u and of v a script accounts for"""
    nu = nv = 0
    for w in words:
        if w == MISMATCHEOP:
            nu, nv = nu + 1, nv + 1
        elif w == DELETIONEOP:
            nu += 1
        elif w == INSERTIONEOP:
            nv += 1
        else:
            nu, nv = nu + w, nv + w
    return nu, nv


def reverse_complement(mapped, orig):
    """initseqinfoRC: makereversecomplement and makereversecomplementorig"""
    m = np.asarray(mapped, np.uint8)[::-1]
    m = np.where(m >= WILDCARD, m, 3 - m).astype(np.uint8)
    table = np.arange(256, dtype=np.uint8)
    for a, b in zip(b"ACGTacgt", b"TGCAtgca"):
        table[a] = b
    return m, table[np.asarray(orig, np.uint8)[::-1]]


def fillthelines(words, u, v):
    first, second = [], []
    i = j = 0
    for w in reversed(words):
        if w == MISMATCHEOP:
            first.append(int(u[i]))
            second.append(int(v[j]))
            i, j = i + 1, j + 1
        elif w == DELETIONEOP:
            first.append(int(u[i]))
            second.append(GAP)
            i += 1
        elif w == INSERTIONEOP:
            first.append(GAP)
            second.append(int(v[j]))
            j += 1
        else:
            assert w & ~MAXIDENTICALLENGTH == 0 and w > 0
            first += [int(c) for c in u[i:i + w]]
            second += [int(c) for c in v[j:j + w]]
            i, j = i + w, j + w
    return first, second


def _origequal(a, b):
    """CHECKORIGEQUAL"""
    if a == b:
        return True
    ca, cb = chr(a), chr(b)
    if a < 128 and ca.islower():
        return b < 128 and ca == cb.lower()
    return b < 128 and ca == cb.upper()


def _editopline(fc, sc, fo, so):
    def differs(x):
        return fc[x] != sc[x] or fc[x] == GAP or fc[x] == WILDCARD
    if not any(differs(x) or not _origequal(fo[x], so[x])
               for x in range(len(fc))):
        return b""
    out = bytearray(b"       ")
    for x in range(len(fc)):
        if differs(x):
            out += b"!"
        else:
            out += b" " if _origequal(fo[x], so[x]) else b"="
    return bytes(out) + b"\n"


def _seqwithgaps(orig):
    return bytes(ord("-") if c == GAP else c for c in orig), \
        sum(1 for c in orig if c == GAP)


def show(words, ucompare, uorig, vcompare, vorig, startfirst, startsecond,
         selfcomparison, linewidth=60):
    """showalignment and the blank line vmatch prints behind it"""
    fc, sc = fillthelines(words, ucompare, vcompare)
    fo, so = fillthelines(words, uorig, vorig)
    assert len(fc) == len(fo)
    out, i, ins1, ins2, n = bytearray(), 0, 0, 0, len(fc)
    while True:
        ln = min(n - i, linewidth)
        text, gaps = _seqwithgaps(fo[i:i + ln])
        ins1 += gaps
        out += b"Sbjct: " + text + b"%*d\n" % (NUMWIDTH + linewidth - ln,
                                               i + startfirst + ln - ins1)
        out += _editopline(fc[i:i + ln], sc[i:i + ln], fo[i:i + ln],
                           so[i:i + ln])
        text, gaps = _seqwithgaps(so[i:i + ln])
        ins2 += gaps
        out += (b"Sbjct: " if selfcomparison else b"Query: ") + text + \
            b"%*d\n" % (NUMWIDTH + linewidth - ln,
                        i + startsecond + ln - ins2)
        i += ln
        if i >= n:
            break
        out += b"\n"
    return bytes(out) + b"\n\n"
