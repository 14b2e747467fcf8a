"""A pure-Python model of vmatch's match selection -- what processfinal
derives from a match (Vmatch/procfinal.c:408-497), assignEvalue with the table
of incprecomputehammingEvalues (procfinal.c:195-257, kurtz/evalues.c:316-426),
matchokay (Vmatch/mokay.c), the best-match list (kurtz/bestmatch.c:33-119) and
the -sort tail (procfinal.c:695-745, kurtz/smcontain.c:23-95,
kurtz/matsort.c) -- floats included: Python's float is the C double, and the
operations below come in the reference's order.

scripts/make_golden_select.py checks this model against the real reference
(order of the lines included) when it writes the fixtures; the tests compare
vsa_select_host and the kernels with it."""

QUERY, SELF, COMPLETE, EDIST, HAMMING = 1, 2, 0, 3, 4   # VSA_SINK_...
SORT_MODES = ("la", "ld", "ia", "id", "ja", "jd", "ea", "ed", "sa", "sd",
              "ida", "idd")
SMALLESTEVALUE = 1.0e-300
AVERAGEQUOT = (0.0, 3.97e+00, 1.28e+01, 3.26e+01, 7.60e+01, 1.71e+02,
               3.77e+02, 8.22e+02, 1.78e+03, 3.91e+03, 8.50e+03, 1.76e+04,
               3.78e+04, 7.98e+04, 1.66e+05, 3.58e+05, 7.44e+05, 1.52e+06,
               3.20e+06, 6.40e+06, 1.31e+07)


class EvalueTable:
    """incprecomputehammingEvalues: line k holds the entries of the lengths
    k + 1, k + 2, ... while they stay above SMALLESTEVALUE"""

    def __init__(self, numofchars):
        self.p = 1.0 / numofchars
        self.first = self.p * ((1.0 - self.p) * (1.0 - self.p))
        self.lines = []

    def line(self, k):
        while len(self.lines) <= k:
            kk = len(self.lines)
            prob, out, l = self.first, [], kk + 1
            self.first *= (((kk + 2) / (kk + 1)) * (1.0 - self.p))
            while prob > SMALLESTEVALUE:
                out.append(prob)
                prob *= ((l + 1) * self.p / (l + 1 - kk))
                l += 1
            self.lines.append(out)
        return self.lines[k]

    def lookup(self, distance, length):
        line = self.line(distance)
        i = length - (distance + 1)
        return line[i] if 0 <= i < len(line) else 0.0


def hequot(d):
    return AVERAGEQUOT[d] if d <= 20 else 1.31e+07 * 2.0 ** (d - 20)


class Layout:
    """the run: kind, alphabet, index and query Multiseq (sequence i of the
    queries starts at the sum of length_j + 1 over j < i)"""

    def __init__(self, kind, totallength, numofchars=4, querylength=(),
                 totalquerylength=0, leastlength=0, noevalue=False,
                 seqoffset=0):
        self.kind, self.totallength = kind, int(totallength)
        self.totalquerylength = int(totalquerylength)
        self.leastlength, self.noevalue = int(leastlength), noevalue
        self.seqoffset = int(seqoffset)
        self.qlen = [int(x) for x in querylength]
        self.qstart, pos = [], 0
        for l in self.qlen:
            self.qstart.append(pos)
            pos += l + 1
        self.table = EvalueTable(numofchars)
        self.dblen = self.totallength - self.totalquerylength - 1


class Values:
    __slots__ = ("length1", "position1", "length2", "position2", "distance",
                 "evalue", "pal")

    @property
    def score(self):
        both = self.length1 + self.length2
        return both - 3 * self.distance if self.distance >= 0 else \
            -(both + 3 * self.distance)

    @property
    def identity(self):
        return 100.0 * (1.0 - abs(self.distance) /
                        max(self.length1, self.length2))

    @property
    def key(self):
        """cmpBestMatch: the smaller tuple is the better match"""
        return (self.evalue, -self.length1, self.position1, -self.length2,
                self.position2, self.pal)


def values(lay, rec, pal):
    """rec: (length, dbstart, queryseq, querystart) of the engine"""
    length, dbstart, queryseq, querystart = (int(x) for x in rec)
    v = Values()
    v.pal = int(bool(pal))
    v.length1, v.position1, v.distance = length, dbstart, 0
    if lay.kind == SELF:
        v.length2, v.position2 = length, queryseq
        if lay.totalquerylength > 0:
            v.position2 -= lay.dblen + 1
            multiplier = float(lay.dblen) * float(lay.totalquerylength)
        else:
            multiplier = 0.5 * float(lay.totallength) * float(lay.totallength)
    else:
        q = queryseq - lay.seqoffset
        seqlen2, seqstart2 = lay.qlen[q], lay.qstart[q]
        if lay.kind == QUERY:
            v.length2, rel = length, querystart
            multiplier = float(lay.totallength) * float(seqlen2)
        else:
            v.length2, rel = seqlen2, 0
            v.distance = {COMPLETE: 0, EDIST: querystart,
                          HAMMING: -querystart}[lay.kind]
            multiplier = float(lay.totallength)
        if pal:
            rel = seqlen2 - (rel + v.length2)
        v.position2 = seqstart2 + rel
    d = v.distance
    lenmatch = v.length2 if (lay.kind in (COMPLETE, EDIST, HAMMING) or
                             d == 0) else max(v.length1, v.length2)
    if lay.noevalue or d > 120:
        v.evalue = 0.0
    elif d <= 0:
        v.evalue = multiplier * lay.table.lookup(-d, lenmatch)
    else:
        v.evalue = multiplier * hequot(d) * lay.table.lookup(d, lenmatch)
    return v


def okay(lay, v, evalue=None, identity=0, leastscore=None, gap=None):
    if v.length1 < lay.leastlength or v.length2 < lay.leastlength:
        return False
    if identity > 0 and v.identity < float(identity):
        return False
    if leastscore is not None and v.score < leastscore:
        return False
    if evalue is not None and v.evalue > evalue:
        return False
    if gap is not None:
        if v.position1 + v.length1 - 1 > v.position2:
            g = -(v.position1 + v.length1 - v.position2)
        else:
            g = v.position2 - (v.position1 + v.length1)
        if g < gap[0] or (len(gap) > 1 and g > gap[1]):
            return False
    return True


def contains(a, b):
    return (a.position1 <= b.position1 and
            b.position1 + b.length1 <= a.position1 + a.length1 and
            a.position2 <= b.position2 and
            b.position2 + b.length2 <= a.position2 + a.length2)


def msort(items, cmp):
    """glibc's qsort, a merge sort: the left run wins where cmp says <= 0.
    The reference's comparison functions are not all consistent (two scores
    of equal absolute value and different sign are each "greater" than the
    other in descending order), so the way of merging is part of the result"""
    n = len(items)
    if n <= 1:
        return list(items)
    a, b = msort(items[:n // 2], cmp), msort(items[n // 2:], cmp)
    out, i, j = [], 0, 0
    while i < len(a) and j < len(b):
        if cmp(a[i], b[j]) <= 0:
            out.append(a[i])
            i += 1
        else:
            out.append(b[j])
            j += 1
    return out + a[i:] + b[j:]


def ordermatchp1l1(p, q):
    """kurtz/smcontain.c:23-34"""
    p, q = p[1], q[1]
    if p.position1 == q.position1:
        if p.length1 == q.length1:
            return 1 if p.position2 > q.position2 else -1
        return 1 if p.length1 > q.length1 else -1
    return 1 if p.position1 > q.position1 else -1


def removecontained(items):
    """items: [(index, Values)] -> (the ones that stay, number removed)"""
    tab = msort(items, ordermatchp1l1)
    n = len(tab)
    reject = [False] * n
    for i in range(n):
        a = tab[i][1]
        j = i - 1
        while j >= 0 and tab[j][1].position1 == a.position1:
            if not reject[i] and contains(a, tab[j][1]):
                reject[j] = True
            j -= 1
        j = i + 1
        while j < n and tab[j][1].position1 <= a.position1 + a.length1:
            if not reject[i] and contains(a, tab[j][1]):
                reject[j] = True
            j += 1
    kept = [t for t, r in zip(tab, reject) if not r]
    return kept, n - len(kept)


def modecmp(mode):
    """the comparison functions of kurtz/matsort.c:28-180"""
    ascend = mode in ("la", "ia", "ja", "ea", "sa", "ida")
    field = {"l": lambda v: v.length1, "i": lambda v: v.position1,
             "j": lambda v: v.position2, "e": lambda v: v.evalue,
             "s": lambda v: v.score, "id": lambda v: v.identity}[mode[:-1]]
    absolute = mode[:-1] in ("s", "id")

    def cmp(p, q):
        x, y = field(p[1]), field(q[1])
        if x == y:
            return 0
        if absolute:            # cmpScoregeneric, cmpIdentitygeneric
            x, y = abs(x), abs(y)
        if ascend:
            return 1 if x > y else -1
        return -1 if x > y else 1
    return cmp


def all_values(lay, recs, flags=None):
    return [values(lay, rec, flags is not None and flags[i])
            for i, rec in enumerate(recs)]


def select(lay, recs, flags=None, best=0, sort=None, vals=None, **filters):
    """-> (indices of the selected records in output order, their E-values,
    stats); flags: the D/P flag per record, or None; vals: all_values() of
    the list, where the caller keeps them for several selections"""
    st = dict(seen=0, rejected=0, duplicates=0, selected=0,
              containedremoved=0)
    items = []
    for i, v in enumerate(vals if vals is not None
                          else all_values(lay, recs, flags)):
        st["seen"] += 1
        if okay(lay, v, **filters):
            items.append((i, v))
        else:
            st["rejected"] += 1
    if best > 0:
        items.sort(key=lambda t: t[1].key)      # stable: first seen first
        out = []
        for t in items:
            if out and out[-1][1].key == t[1].key:
                st["duplicates"] += 1
            elif len(out) == best:
                break
            else:
                out.append(t)
        items = out
        if sort is not None:
            items, st["containedremoved"] = removecontained(items)
            if sort != "ia":
                items = msort(items, modecmp(sort))
    else:
        assert sort is None
    st["selected"] = len(items)
    return [t[0] for t in items], [t[1].evalue for t in items], st
