"""Pure-Python model of the edit-distance extension of exact seeds, vmatch
-l L -e K outside -complete: a literal restatement of editextend with
acceptmatch (kurtz/extendED.c:24-355), extendedleftSEP / extendedrightSEP with
evalentrybackward / evalfrontbackward (kurtz/frontSEP.c:65-339), the front
functions of kurtz/front.gen:48-182 and cmpmatches (include/extcmp.c) on
incgetEvalue (kurtz/evalues.c:382-420), on two Multiseqs given as lists of
ints with their separators.  Literal means: the bounds ubound / vbound are
state that COMPARESYMBOLS moves while the diagonals of a front are evaluated
in ascending order; fronts are narrowed by frontspecparms; MINUSINFINITYFRONT
is the number -max(ulen, vlen); a diagonal on which both texts are the same
place of one array is not slid along; foundseed ends the left side.  Pinned
to recorded runs of the reference by scripts/make_golden_extend_edist.py and
tests/test_extend_edist_host.py; the engine is compared against it."""
import numpy as np

import extend_model as EM

SEPARATOR = EM.SEPARATOR
WILDCARD = EM.WILDCARD
MATCH_DTYPE = EM.MATCH_DTYPE
MAXDISTANCE = 125

# kurtz/evalues.c:59-83
AVERAGEQUOT = [0.0, 3.97e+00, 1.28e+01, 3.26e+01, 7.60e+01, 1.71e+02,
               3.77e+02, 8.22e+02, 1.78e+03, 3.91e+03, 8.50e+03, 1.76e+04,
               3.78e+04, 7.98e+04, 1.66e+05, 3.58e+05, 7.44e+05, 1.52e+06,
               3.20e+06, 6.40e+06, 1.31e+07]
MAXEXPONENTOF2 = 100


def incgetevalue(ev, multiplier, distance, length):
    if distance <= 0:
        return multiplier * ev.lookup(-distance, length)
    if distance > 20:
        if distance - 20 > MAXEXPONENTOF2:
            return 0.0
        hequot = 1.31e+07 * pow(2.0, float(distance - 20))
        return multiplier * hequot * ev.lookup(distance, length)
    return multiplier * AVERAGEQUOT[distance] * ev.lookup(distance, length)


def cmpmatches(ev, dist1, dist2, len1, len2):
    e1 = incgetevalue(ev, 1.0, dist1, len1)
    e2 = incgetevalue(ev, 1.0, dist2, len2)
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


class Frontspec:
    __slots__ = ("offset", "width", "left")

    def __init__(self):
        self.offset = self.width = self.left = 0


class FrontResource:
    """useq, vseq, ubound, vbound are places in the arrays su, sv"""
    __slots__ = ("su", "sv", "useq", "vseq", "ubound", "vbound", "ulen",
                 "vlen", "integermin", "frontspace", "foundseed")


def frontspecparms(gl, fspec, p, r):
    if r <= 0:
        fspec.left = -p
        fspec.width = p + p + 1
    else:
        fspec.left = max(-gl.ulen, -p)
        fspec.width = min(gl.vlen, p) - fspec.left + 1


def accessfront(gl, base, fspec, k):
    """base: the place of diagonal 0 of the front in frontspace"""
    if fspec.left <= k < fspec.left + fspec.width:
        return gl.frontspace[base + k]
    return gl.integermin


def _maximum(gl, fspec, k):
    base = fspec.offset - fspec.left
    t = accessfront(gl, base, fspec, k) + 1
    value = accessfront(gl, base, fspec, k - 1)
    if t < value:
        t = value
    value = accessfront(gl, base, fspec, k + 1) + 1
    if t < value:
        t = value
    return t


def evalentryforward(gl, fspec, k):
    su, sv = gl.su, gl.sv
    t = _maximum(gl, fspec, k)
    if t < 0 or t + k < 0:
        return gl.integermin
    uptr = gl.useq + t
    vptr = gl.vseq + t + k
    if gl.ulen != 0 and gl.vlen != 0:
        if su is sv and uptr == vptr:
            t = gl.ulen - 1
        else:
            while uptr < gl.ubound and vptr < gl.vbound:
                a, b = su[uptr], sv[vptr]
                if a == SEPARATOR:
                    gl.ubound = uptr
                if b == SEPARATOR:
                    gl.vbound = vptr
                if a != b or a >= WILDCARD:
                    break
                uptr += 1
                vptr += 1
            t = uptr - gl.useq
    if gl.useq + t > gl.ubound or gl.vseq + t + k > gl.vbound:
        return gl.integermin
    return t


def evalentrybackward(gl, fspec, k, reachlength):
    su, sv = gl.su, gl.sv
    t = _maximum(gl, fspec, k)
    if t < 0 or t + k < 0:
        return gl.integermin
    if gl.ulen != 0 and gl.vlen != 0:
        uptr = gl.useq - t
        vptr = gl.vseq - (t + k)
        if su is sv and uptr == vptr:
            t = gl.ulen - 1
        else:
            ustart = uptr
            while uptr > gl.ubound and vptr > gl.vbound:
                a, b = su[uptr], sv[vptr]
                if a == SEPARATOR:
                    gl.ubound = uptr
                if b == SEPARATOR:
                    gl.vbound = vptr
                if a != b or a >= WILDCARD:
                    break
                uptr -= 1
                vptr -= 1
            matchlength = ustart - uptr
            if matchlength >= reachlength:
                gl.foundseed = True
                return gl.integermin
            t += matchlength
    if gl.useq - t < gl.ubound or gl.vseq - (t + k) < gl.vbound:
        return gl.integermin
    return t


def evalfront(gl, prevfspec, fspec, r, backward, reachlength):
    defined = False
    for i in range(fspec.width):
        k = fspec.left + i
        if r <= 0 or k <= -r or k >= r:
            if backward:
                v = evalentrybackward(gl, prevfspec, k, reachlength)
            else:
                v = evalentryforward(gl, prevfspec, k)
            if v >= 0:
                defined = True
        else:
            v = gl.integermin
        gl.frontspace.append(v)
    return defined


def _fronts(gl, maxdist, backward, reachlength):
    """-> (number of the last front, [Frontspec])"""
    gl.integermin = -max(gl.ulen, gl.vlen)
    gl.frontspace = [0]
    gl.foundseed = False
    specs = [Frontspec()]
    specs[0].width = 1
    if gl.ulen != gl.vlen or gl.vlen != 0:
        r = 1 - min(gl.ulen, gl.vlen)
        for p in range(1, maxdist + 1):
            fspec = Frontspec()
            fspec.offset = specs[-1].offset + specs[-1].width
            frontspecparms(gl, fspec, p, r)
            specs.append(fspec)
            ret = evalfront(gl, specs[-2], fspec, r, backward, reachlength)
            if backward and ret and gl.foundseed:
                return p, specs
            if not ret:
                return p - 1, specs
            r += 1
        return maxdist, specs
    return 0, specs


def extendedrightSEP(maxdist, su, ustart, ulen, sv, vstart, vlen):
    gl = FrontResource()
    gl.su, gl.sv = su, sv
    gl.ubound = ustart + ulen
    for i in range(min(maxdist + 1, ulen)):
        if su[ustart + i] == SEPARATOR:
            gl.ubound = ustart + i
            break
    gl.vbound = vstart + vlen
    for i in range(min(maxdist + 1, vlen)):
        if sv[vstart + i] == SEPARATOR:
            gl.vbound = vstart + i
            break
    gl.useq, gl.vseq, gl.ulen, gl.vlen = ustart, vstart, ulen, vlen
    h, specs = _fronts(gl, maxdist, False, 0)
    return h, specs, gl.frontspace


def extendedleftSEP(maxdist, su, ulen, sv, vlen, reachlength):
    """useq = su[0 ..], vseq = sv[0 ..]"""
    gl = FrontResource()
    gl.su, gl.sv = su, sv
    gl.ubound = -1
    imin = ulen - maxdist if ulen > maxdist else 0
    for i in range(ulen - 1, imin - 1, -1):
        if su[i] == SEPARATOR:
            gl.ubound = i
            break
    gl.vbound = -1
    imin = vlen - maxdist if vlen > maxdist else 0
    for i in range(vlen - 1, imin - 1, -1):
        if sv[i] == SEPARATOR:
            gl.vbound = i
            break
    gl.useq, gl.vseq, gl.ulen, gl.vlen = ulen - 1, vlen - 1, ulen, vlen
    h, specs = _fronts(gl, maxdist, True, reachlength)
    return h, specs, gl.frontspace


def acceptmatch(distance, length1, pos1, length2, pos2):
    if pos1 >= pos2:
        return False
    if pos1 + length1 - 1 < pos2:
        return True
    if pos1 + length1 >= pos2 + length2:
        return False
    nonoverlap = (pos2 - pos1) + (pos2 + length2) - (pos1 + length1)
    return nonoverlap > distance


def _maxextend(h, specs, space):
    best, nextfront, i = 0, True, h
    while nextfront and i >= 0:
        nextfront = False
        f = specs[i]
        for j in range(f.width):
            v = space[f.offset + j]
            if v < 0:
                nextfront = True
            elif v + f.left + j > best:
                best = v + f.left + j
        i -= 1
    return best


def editextend(ev, querycompare, maxdist, leastlength, seedlength, pos1seed,
               pos2seed, length, seq1, seq2):
    """-> (pos1, pos2, length1, length2, dist) or None"""
    n1, n2 = len(seq1), len(seq2)
    hleft, lspecs, lspace = extendedleftSEP(maxdist, seq1, pos1seed, seq2,
                                            pos2seed, seedlength)
    l1, l2 = pos1seed + length, pos2seed + length
    hright, rspecs, rspace = extendedrightSEP(maxdist, seq1, l1, n1 - l1,
                                              seq2, l2, n2 - l2)
    remain = 0 if length >= leastlength else leastlength - length
    if _maxextend(hleft, lspecs, lspace) + _maxextend(hright, rspecs,
                                                      rspace) < remain:
        return None
    if hleft + hright < maxdist:
        maxdist = hleft + hright
    best = None
    for dist in range(maxdist + 1):
        lookindex = 0 if dist < hright else dist - hright
        while lookindex <= min(dist, hleft):
            lf, rf = lspecs[lookindex], rspecs[dist - lookindex]
            for li in range(lf.width):
                lv = lspace[lf.offset + li]
                if lv < 0:
                    continue
                lk = lf.left + li
                for ri in range(rf.width):
                    rv = rspace[rf.offset + ri]
                    if rv < 0:
                        continue
                    rk = rf.left + ri
                    exti = lv + rv
                    if exti < remain:
                        continue
                    extj = exti + lk + rk
                    if extj < remain:
                        continue
                    pos1 = pos1seed - lv
                    pos2 = pos2seed - lv - lk
                    if querycompare or pos1 <= pos2:
                        length1, length2 = length + exti, length + extj
                    else:
                        pos1, pos2 = pos2, pos1
                        length1, length2 = length + extj, length + exti
                    if seq1[pos1 + length1 - 1] == SEPARATOR:
                        length1 -= 1
                    if seq1[pos1] == SEPARATOR:
                        pos1 += 1
                        length1 -= 1
                    if seq2[pos2 + length2 - 1] == SEPARATOR:
                        length2 -= 1
                    if seq2[pos2] == SEPARATOR:
                        pos2 += 1
                        length2 -= 1
                    if not querycompare and not acceptmatch(
                            dist, length1, pos1, length2, pos2):
                        continue
                    if best is None or cmpmatches(
                            ev, best[4], dist, max(best[2], best[3]),
                            max(length1, length2)) == 1:
                        best = (pos1, pos2, length1, length2, dist)
            lookindex += 1
    return best


def pack(length1, length2, dist):
    return length1 | dist << 48 | ((length2 - length1) & 0xFF) << 56


def extend(seeds, text, numofchars, L, K, S=0, queries=None, evalues=None):
    """seeds, queries as for extend_model.extend -> the records of the
    matches in the order of their seeds: length1 in bits 0-47 of the length,
    the distance in bits 48-55, length2 - length1 as a signed byte above"""
    ev = evalues or EM.Evalues(numofchars)
    seedlength = EM.seedlength_rule(L, K, S)
    seq1 = [int(c) for c in text]
    if queries is None:
        seq2, qstart = seq1, None
    else:
        seq2, qstart = EM.multiseq(*queries)
    out = []
    for m in seeds:
        length, pos1 = int(m["length"]), int(m["dbstart"])
        if queries is None:
            pos2 = int(m["queryseq"])
        else:
            pos2 = qstart[int(m["queryseq"])] + int(m["querystart"])
        best = editextend(ev, queries is not None, K, L, seedlength, pos1,
                          pos2, length, seq1, seq2)
        if best is None:
            continue
        p1, p2, length1, length2, dist = best
        if queries is None:
            out.append((pack(length1, length2, dist), p1, p2, 0))
        else:
            rel = (int(m["querystart"]) - (pos2 - p2)) & ((1 << 64) - 1)
            out.append((pack(length1, length2, dist), p1,
                        int(m["queryseq"]), rel))
    res = np.zeros(len(out), MATCH_DTYPE)
    for i, o in enumerate(out):
        res[i] = o
    return res


def lengths1(rec):
    return rec["length"] & np.uint64((1 << 48) - 1)


def distances(rec):
    return (rec["length"] >> np.uint64(48)) & np.uint64(0xFF)


def lengths2(rec):
    diff = (rec["length"] >> np.uint64(56)).astype(np.uint8).astype(np.int8)
    return (lengths1(rec).astype(np.int64) +
            diff.astype(np.int64)).astype(np.uint64)
