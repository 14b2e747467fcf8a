"""The recorded runs of vmatch -l L -e K outside -complete
(tests/golden/extend_edist_manifest.json, extend_edist_expected.npz, written
by scripts/make_golden_extend_edist.py) -- the recipes of extend_cases.RUNS
with -h replaced by -e -- and the seed lists made by hand for the border
cases of the edit-distance extension.  Shared by the generator and the two
extend_edist test modules."""
import json
import os

import numpy as np

import extend_cases as EC
import extend_edist_model as DM
import helpers as H

RUNS = [dict(r, key=r["key"].replace("_h", "_e")) for r in EC.RUNS]

load, passes, oracle_seeds, md5 = EC.load, EC.passes, EC.oracle_seeds, EC.md5


def run_of(key):
    return next(r for r in RUNS if r["key"] == key)


def vmatch_args(r):
    return ["-e" if a == "-h" else a for a in EC.vmatch_args(r)]


def parse_rows(lines):
    """the default columns -> rows (length1, seq1, rel1, length2, seq2, rel2,
    distance, palindromic)"""
    out = np.zeros((len(lines), 8), np.int64)
    for i, l in enumerate(lines):
        f = l.split()
        out[i] = (int(f[0]), int(f[1]), int(f[2]), int(f[4]), int(f[5]),
                  int(f[6]), int(f[7]), 1 if f[3] == "P" else 0)
    return out


def rows_of(r, rec, palindromic):
    """records of the engine -> rows as vmatch prints them"""
    idx, q = load(r)
    rec = np.asarray(rec)
    out = np.zeros((len(rec), 8), np.int64)
    length2 = DM.lengths2(rec).astype(np.int64)
    out[:, 0] = DM.lengths1(rec)
    out[:, 1], out[:, 2] = idx.seq_rel(rec["dbstart"])
    out[:, 3] = length2
    out[:, 6] = DM.distances(rec)
    out[:, 7] = palindromic
    if r["q"]:
        out[:, 4] = rec["queryseq"]
        rel = rec["querystart"].astype(np.int64)
        if palindromic:
            qlen = q.length.astype(np.int64)[rec["queryseq"].astype(np.int64)]
            rel = qlen - (rel + length2)
        out[:, 5] = rel
    else:
        s2, r2 = idx.seq_rel(rec["queryseq"])
        out[:, 4] = s2.astype(np.int64) - (idx.numofdbsequences
                                           if idx.hasqueries else 0)
        out[:, 5] = r2
    return out


def sink_kwargs(V, r, palindromic):
    kw = EC.sink_kwargs(V, r, palindromic)
    kw["kind"] = V.SINK_QUERY_EDIST if r["q"] else V.SINK_SELF_EDIST
    return kw


_manifest = None
_arrays = None


def manifest():
    global _manifest
    if _manifest is None:
        with open(os.path.join(H.GOLDEN, "extend_edist_manifest.json")) as f:
            _manifest = json.load(f)
    return _manifest


def expected_rows(key):
    global _arrays
    if _arrays is None:
        _arrays = np.load(os.path.join(H.GOLDEN, "extend_edist_expected.npz"))
    return _arrays[key].astype(np.int64).reshape(-1, 8)


def golden_keys(error=False):
    return [r["key"] for r in RUNS if r["error"] == error]


# --------------------------------------------------------------------------
# seed lists made by hand: the border cases of the extension
# --------------------------------------------------------------------------

SEP, WILD = H.SEPARATOR, H.WILDCARD


class Scenario:
    """A text, a batch of edited copies of its windows (or none: seeds of the
    text against itself) and a list of seeds on exact stretches.  A read is
    made of the symbols left of the seed, the seed and the symbols right of
    it; edits are given by their distance from the seed: (d, "s") a
    substitution of the symbol d places away, (d, "i") a symbol inserted into
    the read there, (d, "d") the symbol deleted from it, (d, "S") / (d, "W")
    a separator / wildcard put over it."""

    def __init__(self, name, n, rngseed, dense=False):
        self.name = name
        self.rng = np.random.default_rng(rngseed)
        self.text = self.rng.integers(0, 4, n).astype(np.uint8)
        self.reads, self.seeds, self.dense = [], [], dense
        self.params = []     # [(L, K, S)]

    def other(self, c):
        return (int(c) + 1 + int(self.rng.integers(0, 3))) % 4

    def edited(self, part, edits):
        """part: the symbols of a side in the order away from the seed"""
        out = [int(c) if c < 4 else 0 for c in part]
        for d, what in sorted(edits, reverse=True):
            if d >= len(out):
                continue
            if what == "s":
                out[d] = self.other(out[d])
            elif what == "i":
                out.insert(d, self.other(out[d]))
            elif what == "d":
                del out[d]
            elif what == "S":
                out[d] = SEP
            elif what == "W":
                out[d] = WILD
        return out

    def planted(self, w, A, s, B, left=(), right=(), beside=True):
        """a read whose seed of s symbols is text[w + A : w + A + s], with A
        symbols of the text left of it and B right of it before the edits;
        beside: the symbols directly beside the seed are substituted, so that
        the seed is maximal -> the number of the read"""
        t = self.text
        lpart = list(t[w:w + A][::-1])
        rpart = list(t[w + A + s:w + A + s + B])
        le = list(left) + ([(0, "s")] if beside and A > 0 else [])
        re = list(right) + ([(0, "s")] if beside and B > 0 else [])
        lq = self.edited(lpart, le)
        rq = self.edited(rpart, re)
        mid = [int(c) if c < 4 else 0 for c in t[w + A:w + A + s]]
        q = np.array(lq[::-1] + mid + rq, np.uint8)
        self.reads.append(q)
        self.seeds.append((s, w + A, len(self.reads) - 1, len(lq)))
        return len(self.reads) - 1

    def seed(self, qi, o, s, dbstart):
        self.seeds.append((s, dbstart, qi, o))

    def selfseed(self, p1, p2, s):
        self.seeds.append((s, p1, p2, 0))

    def records(self):
        rec = np.zeros(len(self.seeds), H.MATCH_DTYPE)
        for i, x in enumerate(self.seeds):
            rec[i] = x
        return rec

    def queries(self):
        """the batch (H.Queries) or None"""
        if not self.reads:
            return None
        if self.dense:
            m = len(self.reads[0])
            assert all(len(q) == m for q in self.reads)
            return H.Queries.uniform(np.concatenate(self.reads), m)
        return H.Queries.from_list(self.reads)

    def triple(self):
        q = self.queries()
        return None if q is None else (q.symbols, q.start, q.length)

    def model(self, L, K, S):
        return DM.extend(self.records(), self.text, 4, L, K, S, self.triple())


KS = (1, 2, 5, 8, 16, 31)


def _borders(dense):
    """seeds beginning at text and batch positions 0 .. K + 1 and ending at
    the last K + 1 positions (narrowed fronts, r > 0), both sides empty;
    first, middle and last read of a ragged / dense batch"""
    n = 700
    sc = Scenario("borders_dense" if dense else "borders", n,
                  21 if dense else 22, dense)
    if dense:
        m = 48
        for w in (0, 0, 130, 301, n - m, n - m):
            q = sc.text[w:w + m].copy()
            for o in (9, 23, 29, 37):
                q[o] = sc.other(q[o])
            sc.reads.append(q)
            qi = len(sc.reads) - 1
            for o in (0, 1, 2, 3, 4, 10):
                sc.seed(qi, o, 5, w + o)
            for e in (m, m - 1, m - 2, m - 3, m - 4, m - 12):
                sc.seed(qi, e - 5, 5, w + e - 5)
        # a read that is one seed: both sides empty in the batch
        sc.params = [(10, 2, 0), (14, 5, 0), (6, 1, 0), (12, 8, 0)]
        return sc
    for w, length in ((0, 60), (0, 31), (200, 47), (n - 60, 60), (n - 33, 33),
                      (1, 40), (n - 41, 40)):
        q = sc.text[w:w + length].copy()
        for o in (9, 17, length // 2 + 3, length - 11):
            q[o] = sc.other(q[o])
        sc.reads.append(q)
        qi = len(sc.reads) - 1
        for o in (0, 1, 2, 3, 4, 11):
            sc.seed(qi, o, 4, w + o)
        for e in (length, length - 1, length - 2, length - 3, length - 5):
            sc.seed(qi, e - 4, 4, w + e - 4)
    # the whole text as a read: both sides empty on both Multiseqs when it
    # is alone; here the first read of one and the text
    sc.reads.append(sc.text[0:6].copy())
    sc.seed(len(sc.reads) - 1, 0, 6, 0)
    # the read longer than the text copy on either side
    pre = sc.rng.integers(0, 4, 7).astype(np.uint8)
    sc.reads.append(np.concatenate((pre, sc.text[0:30], pre)))
    for o in (0, 1, 2, 3):
        sc.seed(len(sc.reads) - 1, 7 + o, 5, o)
    sc.reads.append(np.concatenate((pre, sc.text[n - 30:n], pre)))
    for e in (0, 1, 2, 3):
        sc.seed(len(sc.reads) - 1, 7 + 30 - 5 - e, 5, n - 5 - e)
    # short reads at the very start of the batch Multiseq: vlen < K
    sc.params = [(10, 2, 0), (14, 5, 0), (6, 1, 0), (12, 8, 0), (12, 16, 0)]
    return sc


def _bothempty():
    """a text and a batch that are one seed: no front but front 0"""
    sc = Scenario("bothempty", 12, 23)
    sc.reads.append(sc.text.copy())
    sc.seed(0, 0, 12, 0)
    sc.params = [(10, 2, 0), (12, 1, 0), (13, 3, 0)]
    return sc


def _specials():
    """a separator or a wildcard 1, 2, 3, K, K + 1, K + 2 and 17 symbols from
    the seed, in the text only, in the read only, in both at different
    distances, on each side (K = 5: the pre-scan window ends at 5 / 6)"""
    sc = Scenario("specials", 4000, 24)
    t = sc.text
    ds = (1, 2, 3, 5, 6, 7, 17)
    w = 40
    for d in ds:
        # in the text: right of a seed, left of another
        t[w + 30 + 8 + d] = SEP
        sc.planted(w, 30, 8, 30, [(3, "s")], [(d + 2, "s")])
        t[w + 100 - d - 1] = SEP
        sc.planted(w + 70, 30, 8, 30, [(d + 3, "s")], [(4, "i")])
        w += 150
    for d in ds:
        for what in ("S", "W"):
            # in the read only
            sc.planted(w, 30, 8, 30, [(2, "d")], [(d, what)])
            sc.planted(w, 30, 8, 30, [(d, what)], [(2, "i")])
            # a candidate that ends / begins on the separator
            sc.planted(w, 30, 8, 30, [(d, what)], [(d + 1, what)],
                       beside=False)
        w += 80
    for d in ds:
        # in both, at different distances, and facing each other
        t[w + 30 + 8 + d] = SEP
        sc.planted(w, 30, 8, 30, [], [(d + 2, "S"), (1, "d")])
        sc.planted(w, 30, 8, 30, [], [(max(d - 1, 1), "S")])
        sc.planted(w, 30, 8, 30, [], [(d, "S")])
        t[w + 90] = WILD
        sc.planted(w + 60, 20, 8, 30, [], [(d, "W")])
        w += 150
    assert w < 4000
    sc.params = [(12, 5, 0), (10, 2, 0), (10, 1, 0), (12, 8, 0)]
    return sc


def _indels():
    """an insertion, a deletion and a substitution directly beside the seed
    and 2, 5 and 9 symbols away, on each side; two adjacent indels; an indel
    inside a homopolymer run; an insertion left and a deletion right"""
    sc = Scenario("indels", 3000, 25)
    t = sc.text
    t[1000:1012] = 2           # homopolymer runs
    t[1040:1052] = 1
    for d in (0, 2, 5, 9):
        for what in ("i", "d", "s"):
            sc.planted(100, 40, 10, 40, [(d, what)], [], beside=d != 0)
            sc.planted(100, 40, 10, 40, [], [(d, what)], beside=d != 0)
            sc.planted(300, 40, 10, 40, [(d, what)], [(d + 1, what)],
                       beside=d != 0)
    for pair in ("ii", "dd", "id", "di"):
        sc.planted(500, 40, 10, 40, [(4, pair[0]), (5, pair[1])], [])
        sc.planted(500, 40, 10, 40, [], [(4, pair[0]), (5, pair[1])])
    for what in ("i", "d"):
        # the run right of a seed and left of another
        sc.planted(950, 40, 10, 60, [], [(5, what)])
        sc.planted(950, 40, 10, 60, [], [(3, what), (8, what)])
        sc.planted(1012, 0, 10, 40, [], [])
        sc.planted(1052, 40, 10, 40, [(4, what)], [])
    # lk + rk = 0 while exti is short of remain: few symbols on each side
    for a, b in ((6, 6), (8, 4), (4, 8), (10, 10)):
        sc.planted(1500, a, 10, b, [(2, "i")], [(2, "d")])
        sc.planted(1500, a, 10, b, [(2, "d")], [(2, "i")])
    sc.params = [(30, 2, 0), (40, 5, 0), (20, 1, 0), (26, 3, 0), (50, 8, 0)]
    return sc


def _stoprule():
    """exact stretches of seedlength - 1, seedlength and seedlength + 1
    behind the first error on the left (L = 60, K = 2: seedlength 20), where
    the side ends, and on the right, where no rule applies; and a -seedlength
    nothing reaches"""
    sc = Scenario("stoprule", 900, 26)
    for first in (1, 4, 9):
        for gap in (19, 20, 21, 22):
            for what in ("s", "i", "d"):
                sc.planted(100, 120, 20, 120,
                           [(first, what), (first + gap, "s"),
                            (first + gap + 7, "s")], [])
                sc.planted(100, 120, 20, 120, [],
                           [(first, what), (first + gap, "s"),
                            (first + gap + 7, "s")])
    sc.params = [(60, 2, 0), (60, 5, 0), (60, 2, 100000), (40, 1, 0)]
    return sc


def _fewerrors():
    """hleft + hright < K; a seed of length >= L (remain = 0); sides that end
    at read borders after 0 - 3 symbols; matches longer than the E-value
    table, so that identity, then length, then "later wins" decide"""
    sc = Scenario("fewerrors", 2600, 27)
    for A, B in ((0, 0), (1, 1), (2, 2), (3, 9), (9, 3), (12, 12), (0, 14),
                 (3, 0)):
        sc.planted(300 + A, A, 30, B, [(4, "i")] if A > 8 else [],
                   [(5, "d")] if B > 8 else [])
    for s in (40, 41, 60):
        sc.planted(500, 25, s, 25, [(3, "i"), (12, "s")],
                   [(2, "d"), (9, "s"), (17, "i")])
    sc.planted(1000, 400, 30, 420, [(100, "i"), (250, "s"), (390, "d")],
               [(120, "d"), (300, "i"), (410, "s")])
    sc.planted(1000, 400, 30, 420, [(390, "i")], [])
    sc.planted(1700, 320, 25, 330, [], [(40, "d"), (300, "i")])
    # (L = 700 with a seed length nothing reaches: without it the stop rule
    # ends the left side on the first long exact stretch and nothing reaches
    # 700; every candidate of such a match has the E-value 0.0)
    sc.params = [(40, 5, 0), (40, 2, 0), (30, 1, 0), (700, 5, 100000),
                 (40, 31, 0)]
    return sc


TIES = (700, 5, 100000)   # the parameter set of fewerrors whose matches tie


def _selfseeds():
    """seeds of a text against itself: planted repeats with indels; pairs
    less than K + 2 apart (the same-text shortcut, acceptmatch); pairs given
    with position1 > position2 (the swap); a separator between the instances"""
    sc = Scenario("selfseeds", 3000, 28)
    t = sc.text
    t[1500] = SEP
    for a, b, m in ((0, 1501, 300), (400, 2000, 350), (800, 2600, 380)):
        m = min(m, len(t) - b - 20, 1500 - a)
        copy = sc.edited(list(t[a:a + m]),
                         [(int(x), "sid"[int(x) % 3]) for x in
                          np.cumsum(sc.rng.integers(9, 40, 20)) if x < m - 5])
        t[b:b + len(copy)] = copy
        # the exact stretches of the two copies, found by alignment-free
        # search: every 8-mer of the first at the places it has in the second
        for o in range(0, m - 8, 5):
            for shift in range(-6, 7):
                p2 = b + o + shift
                if p2 + 8 <= len(t) and np.array_equal(t[a + o:a + o + 8],
                                                       t[p2:p2 + 8]):
                    sc.selfseed(a + o, p2, 8)
                    if o % 3 == 0:
                        sc.selfseed(p2, a + o, 8)
    # a tandem of period 3 and a run of one symbol: pairs with position2 -
    # position1 = 1 .. 9, K + 1 for the largest K of the parameter sets
    t[1200:1260] = np.tile(t[1200:1203], 20)
    for d in (3, 6):
        for p in (1205, 1210, 1230):
            sc.selfseed(p, p + d, 9)
    t[1300:1340] = 3
    for d in (1, 2, 4, 5, 7, 8, 9):
        sc.selfseed(1305, 1305 + d, 12)
        sc.selfseed(1305 + d, 1305, 12)
    sc.params = [(16, 2, 0), (20, 5, 0), (12, 1, 0), (24, 8, 0)]
    return sc


def _words(budget):
    """all 64 combinations of dbstart % 8 and the query address % 8; the
    error that ends a slide at offsets 7 .. 17 and around the lane budget, on
    the main diagonal and on a diagonal reached after an indel"""
    ctx = budget + 40
    sc = Scenario("words", 2 * ctx + 700, 29)
    places = [7, 8, 9, 15, 16, 17, budget - 9, budget - 8, budget - 1, budget,
              budget + 1, budget + 7, budget + 8]
    for T in places:
        sc.planted(50, ctx, 12, 10, [(T, "s")], [])
        sc.planted(50 + ctx, 10, 12, ctx, [], [(T, "s")])
        sc.planted(50, ctx, 12, 10, [(1, "i"), (T + 2, "s")], [])
        sc.planted(50 + ctx, 10, 12, ctx, [], [(1, "d"), (T + 2, "s")])
    base = 2 * ctx + 100
    for i in range(8):
        # (63 symbols and a separator: every read begins at the same address
        # modulo 8, its window of the text one symbol further on)
        q = sc.text[base + i:base + i + 63].copy()
        for o in (5, 44):
            q[o] = sc.other(q[o])
        sc.reads.append(q)
        for o in range(20, 28):
            sc.seed(len(sc.reads) - 1, o, 4, base + i + o)
    sc.params = [(30, 2, 100000), (30, 2, 0), (30, 1, 100000), (30, 5, 100000)]
    return sc


def residues(sc):
    q = sc.queries()
    return {(int(d) % 8, (int(q.start[int(qi)]) + int(o)) % 8)
            for _, d, qi, o in sc.seeds[-64:]}


def _everywidth():
    """one planted repeat family for K = 1, 2, 5, 8, 16, 31: every group
    width, errors spread so that many fronts are defined"""
    sc = Scenario("everywidth", 1600, 30)
    for w in (100, 700):
        for step in (9, 14):
            edits = [(int(x), "sid"[i % 3]) for i, x in
                     enumerate(range(3, 220, step))]
            sc.planted(w, 230, 12, 230, edits, edits[1:])
    sc.params = [(40, K, 0) for K in KS]
    return sc


def _boundsorder():
    """two seeds whose match depends on the literal order of the bounds.
    Both: two symbols deleted directly left of the seed, so that only left
    entries on diagonal -2 reach L, and a candidate needs a right entry on
    diagonal 2; u ends at a separator 30 symbols right of the seed, the read
    one symbol later, and the right entry on diagonal 2 lies behind the
    read's separator.  First seed: the slides never look at that separator,
    the diagonal steps over it -- with "first separator of the side" as the
    bound there is no match.  Second seed, in a run of one symbol: diagonal 0
    finds u's separator in front 1, and diagonal 1 of the SAME front then
    stops at it without reading the read's separator; evaluated under the
    bounds of the start of the front it would read it, and there is no
    match."""
    sc = Scenario("boundsorder", 700, 31)
    t = sc.text
    filler = sc.rng.integers(1, 4, 30).astype(np.uint8)
    for s0, run in ((200, False), (500, True)):
        if run:
            t[s0 + 12:s0 + 12 + 34] = 0
        x = t.copy()
        t[s0 + 12 + 30] = SEP
        left = list(x[s0 - 2 - 50:s0 - 2])
        right = list(x[s0 + 12:s0 + 12 + 30]) + \
            [0 if run else (int(x[s0 + 12 + 30]) + 1) % 4]
        sc.reads.append(np.array(left + list(x[s0:s0 + 12]) + right,
                                 np.uint8))
        sc.seed(len(sc.reads) - 1, len(left), 12, s0)
        sc.reads.append(filler)
    sc.params = [(94, 6, 100000), (95, 6, 100000), (94, 4, 100000),
                 (90, 5, 100000)]
    return sc


def scenarios(lane_budget):
    """name -> Scenario; the limit is the one the library exports"""
    out = [_borders(False), _borders(True), _bothempty(), _specials(),
           _indels(), _stoprule(), _fewerrors(), _selfseeds(),
           _words(lane_budget), _everywidth(), _boundsorder()]
    return {sc.name: sc for sc in out}


SCENARIOS = ("borders", "borders_dense", "bothempty", "specials", "indels",
             "stoprule", "fewerrors", "selfseeds", "words", "everywidth",
             "boundsorder")
