"""The recorded runs of vmatch -s (tests/golden/align_manifest.json,
align_expected.npz, written by scripts/make_golden_align.py): the recipes,
the texts with their original characters, the conversion between the rows
vmatch prints and the records of the engine, the two substrings a record
names -- and the match lists made by hand for the border cases of the
alignment.  Shared by the generator and the two align test modules."""
import gzip
import hashlib
import json
import os

import numpy as np

import align_model as AM
import helpers as H

SEP, WILD = H.SEPARATOR, H.WILDCARD

# sink kinds (include/vstree_amd.h)
COMPLETE, QUERY, SELF, APPROX_EDIST, APPROX_HAMMING = 0, 1, 2, 3, 4
QUERY_HAMMING, SELF_HAMMING, QUERY_EDIST, SELF_EDIST = 8, 9, 10, 11
SELFKINDS = (SELF, SELF_HAMMING, SELF_EDIST)

# name -> (database file, query file) under tests/golden
CASES = {
    "at1mb": ("at1MB.gz", None),
    "c6": ("c6_db.fna.gz", "c6_reads.fna.gz"),
    "micro": ("micro_db.fna", "micro_q.fna"),
    "wildcards": ("Wildcards.fna", "Wildcards.fna"),
    "tandem": ("align_tandem.fna", None),
}


def R(key, case, kind, args, width, strands="d"):
    return dict(key=key, case=case, kind=kind, args=args, width=width,
                strands=strands, q=kind not in SELFKINDS)


# args: what stands between `vmatch` and `-s W`; width 0: -s alone (60)
RUNS = [
    R("at1mb_l40_e2_s60", "at1mb", SELF_EDIST, ["-l", "40", "-e", "2"], 60),
    R("at1mb_l30_h2_s50", "at1mb", SELF_HAMMING, ["-l", "30", "-h", "2"], 50),
    R("at1mb_l32_s70", "at1mb", SELF, ["-l", "32"], 70),
    R("c6_q_l25_e2_dp_s40", "c6", QUERY_EDIST,
      ["-l", "25", "-e", "2", "-d", "-p"], 40, "dp"),
    R("c6_q_l20_h2_dp_s", "c6", QUERY_HAMMING,
      ["-l", "20", "-h", "2", "-d", "-p"], 0, "dp"),
    R("c6_complete_e1_s", "c6", APPROX_EDIST, ["-complete", "-e", "1"], 0),
    R("c6_complete_h1_s", "c6", APPROX_HAMMING, ["-complete", "-h", "1"], 0),
    R("c6_complete_s", "c6", COMPLETE, ["-complete"], 0),
    R("c6_q_l30_s70", "c6", QUERY, ["-l", "30"], 70),
    R("micro_q_l8_e1_s30", "micro", QUERY_EDIST, ["-l", "8", "-e", "1"], 30),
    R("wildcards_q_l8_h1_dp_s", "wildcards", QUERY_HAMMING,
      ["-l", "8", "-h", "1", "-d", "-p"], 0, "dp"),
    R("wildcards_l6_e1_s20", "wildcards", SELF_EDIST, ["-l", "6", "-e", "1"],
      20),
    # overlapping self matches: the same-text shortcut of front.gen:120
    R("tandem_l20_e2_s", "tandem", SELF_EDIST, ["-l", "20", "-e", "2"], 0),
]


def run_of(key):
    return next(r for r in RUNS if r["key"] == key)


def vmatch_args(r):
    return r["args"] + ["-s"] + ([str(r["width"])] if r["width"] else [])


def md5(text):
    return hashlib.md5(text).hexdigest()


class Text:
    """the sequences of a FASTA file as the reference's Multiseq: mapped
    symbols and original characters with a separator between two sequences,
    where the sequences begin and how long they are"""

    def __init__(self, path):
        opener = gzip.open if path.endswith(".gz") else open
        with opener(path, "rb") as f:
            raw = f.read()
        seqs = [b"".join(x.replace(b" ", b"") for x in rec.split(b"\n")[1:])
                for rec in raw.split(b">")[1:]]
        symmap = H.dna_map()
        self.orig = np.frombuffer(bytes([SEP]).join(seqs), np.uint8).copy()
        self.length = np.array([len(s) for s in seqs], np.uint64)
        self.start = np.concatenate(
            ([0], np.cumsum(self.length + np.uint64(1))[:-1])).astype(
                np.uint64)
        self.symbols = symmap[self.orig]
        self.symbols[(self.start[1:] - np.uint64(1)).astype(np.int64)] = SEP
        assert not (self.symbols == 253).any()
        self.markpos = (self.start[1:] - np.uint64(1)).astype(np.uint64)
        self.n = len(self.symbols)


_texts = {}


def load(case):
    """-> (Text of the database, Text of the queries or None)"""
    if case not in _texts:
        db, q = CASES[case]
        _texts[case] = (Text(os.path.join(H.GOLDEN, db)),
                        None if q is None else Text(os.path.join(H.GOLDEN, q)))
    return _texts[case]


# --------------------------------------------------------------------------
# rows <-> records
# --------------------------------------------------------------------------

def parse_rows(lines):
    """match lines -> rows (length1, seq1, rel1, length2, seq2, rel2,
    distance, palindromic)"""
    out = np.zeros((len(lines), 8), np.int64)
    for i, l in enumerate(lines):
        f = l.split()
        out[i] = (int(f[0]), int(f[1]), int(f[2]), int(f[4]), int(f[5]),
                  int(f[6]), int(f[7]), 1 if f[3] == "P" else 0)
    return out


def records_of(r, rows):
    """rows of ONE pass (all direct or all palindromic) -> the records the
    engine delivers for them"""
    db, q = load(r["case"])
    rows = np.asarray(rows, np.int64)
    rec = np.zeros(len(rows), H.MATCH_DTYPE)
    kind = r["kind"]
    len1, len2, dist = rows[:, 0], rows[:, 3], rows[:, 6]
    rec["dbstart"] = db.start[rows[:, 1]].astype(np.int64) + rows[:, 2]
    if kind in SELFKINDS:
        rec["queryseq"] = db.start[rows[:, 4]].astype(np.int64) + rows[:, 5]
    else:
        rec["queryseq"] = rows[:, 4]
        rel = rows[:, 5].copy()
        pal = rows[:, 7] != 0
        rel[pal] = (q.length[rows[:, 4]].astype(np.int64) -
                    (rel + len2))[pal]
        rec["querystart"] = rel
    if kind in (QUERY_EDIST, SELF_EDIST):
        rec["length"] = (len1.astype(np.uint64) |
                         dist.astype(np.uint64) << np.uint64(48) |
                         ((len2 - len1) & 0xFF).astype(np.uint64)
                         << np.uint64(56))
    elif kind in (QUERY_HAMMING, SELF_HAMMING):
        rec["length"] = len1.astype(np.uint64) | \
            (-dist).astype(np.uint64) << np.uint64(48)
    else:
        rec["length"] = len1
        if kind in (APPROX_EDIST, APPROX_HAMMING):
            assert (rec["querystart"] == 0).all()
            rec["querystart"] = np.abs(dist)
    return rec


def passes(r, rows):
    """[(palindromic, the rows of that pass)] in the order of the output"""
    rows = np.asarray(rows)
    out = []
    for pal in ([0] if "d" in r["strands"] else []) + \
            ([1] if "p" in r["strands"] else []):
        out.append((pal, rows[rows[:, 7] == pal]))
    assert sum(len(x) for _, x in out) == len(rows)
    # (-d -p prints the direct matches first)
    assert np.array_equal(np.concatenate([x for _, x in out]), rows)
    return out


def sink_kwargs(V, r, palindromic, **more):
    db, q = load(r["case"])
    kw = dict(kind=r["kind"], totallength=db.n, markpos=db.markpos,
              numofchars=4, palindromic=bool(palindromic))
    if r["q"]:
        kw.update(querystart=q.start, querylength=q.length,
                  querytotallength=q.n)
    kw.update(more)
    return kw


# --------------------------------------------------------------------------
# what a record names (the model's side of align_rules.h)
# --------------------------------------------------------------------------

def view(kind, rec, qlength=None):
    """-> (length1, length2, position2 or start in the query sequence,
    stored distance: negative for Hamming)"""
    length, qs = int(rec["length"]), int(rec["querystart"])
    if kind in (QUERY_EDIST, SELF_EDIST):
        len1 = length & ((1 << 48) - 1)
        diff = length >> 56
        len2 = len1 + (diff - 256 if diff >= 128 else diff)
        dist = (length >> 48) & 0xFF
    elif kind in (QUERY_HAMMING, SELF_HAMMING):
        len1 = len2 = length & ((1 << 48) - 1)
        dist = -(length >> 48)
    elif kind in (COMPLETE, APPROX_EDIST, APPROX_HAMMING):
        len1, len2 = length, int(qlength)
        dist = {COMPLETE: 0, APPROX_EDIST: qs, APPROX_HAMMING: -qs}[kind]
        qs = 0
    else:
        len1 = len2 = length
        dist = 0
    return len1, len2, (int(rec["queryseq"]) if kind in SELFKINDS else qs), \
        dist


class Pair:
    """the two substrings of a record as the reference hands them to
    shownormalstringout, and where showalignment says they begin"""

    def __init__(self, kind, rec, palindromic, text, orig, markpos, qtriple):
        seq2 = int(rec["queryseq"])
        qlen = None if kind in SELFKINDS else int(qtriple[2][seq2])
        len1, len2, p2, self.distance = view(kind, rec, qlen)
        p1 = int(rec["dbstart"])
        starts = np.concatenate(([0], np.asarray(markpos, np.int64) + 1))
        s1 = int(np.searchsorted(np.asarray(markpos, np.int64), p1, "right"))
        self.u, self.uorig = text[p1:p1 + len1], orig[p1:p1 + len1]
        self.startfirst = p1 - int(starts[s1])
        self.sametext = None
        self.selfcomparison = kind in SELFKINDS
        if self.selfcomparison:
            s2 = int(np.searchsorted(np.asarray(markpos, np.int64), p2,
                                     "right"))
            self.v, self.vorig = text[p2:p2 + len2], orig[p2:p2 + len2]
            self.startsecond = p2 - int(starts[s2])
            self.sametext = p2 - p1
            return
        qsym, qstart, _, qorig = qtriple
        rel = qlen - (p2 + len2) if palindromic else p2
        a = int(qstart[seq2]) + rel
        self.v, self.vorig = qsym[a:a + len2], qorig[a:a + len2]
        if palindromic:
            self.v, self.vorig = AM.reverse_complement(self.v, self.vorig)
        self.startsecond = rel

    def script(self):
        return AM.script(self.u, self.v, self.distance, self.sametext)

    def show(self, words, linewidth):
        return AM.show(words, self.u, self.uorig, self.v, self.vorig,
                       self.startfirst, self.startsecond,
                       self.selfcomparison, linewidth or 60)


def pairs_of(r, rec, palindromic):
    db, q = load(r["case"])
    qt = None if q is None or not r["q"] else (q.symbols, q.start, q.length,
                                               q.orig)
    return [Pair(r["kind"], x, palindromic, db.symbols, db.orig, db.markpos,
                 qt) for x in rec]


def csr(scripts):
    """a list of scripts -> (offsets[n + 1], words) as the entries give them"""
    offsets = np.zeros(len(scripts) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in scripts])
    words = np.array([w for s in scripts for w in s], np.uint16)
    return offsets, words


# --------------------------------------------------------------------------
# fixtures
# --------------------------------------------------------------------------

_manifest = None
_arrays = None


def manifest():
    global _manifest
    if _manifest is None:
        with open(os.path.join(H.GOLDEN, "align_manifest.json")) as f:
            _manifest = json.load(f)["runs"]
    return _manifest


def expected(key, what):
    """what: rows, offsets, words"""
    global _arrays
    if _arrays is None:
        _arrays = np.load(os.path.join(H.GOLDEN, "align_expected.npz"))
    a = _arrays["%s__%s" % (key, what)]
    if what == "rows":
        return a.astype(np.int64).reshape(-1, 8)
    return a.astype(np.uint64 if what == "offsets" else np.uint16)


# --------------------------------------------------------------------------
# match lists made by hand: the border cases of the alignment
# --------------------------------------------------------------------------

LETTERS = np.full(256, SEP, np.uint8)
LETTERS[:4] = np.frombuffer(b"acgt", np.uint8)
LETTERS[WILD] = ord("n")


def rc(symbols):
    s = np.asarray(symbols, np.uint8)[::-1]
    return np.where(s >= WILD, s, 3 - s).astype(np.uint8)


def edited(u, edits):
    """u with edits [(position in u, "s" | "i" | "d" | "w")] applied: a
    substitution, a symbol inserted in front of the position, the symbol
    deleted, a wildcard put over it"""
    out = [int(c) for c in u]
    for pos, what in sorted(edits, reverse=True):
        if what == "s":
            out[pos] = (out[pos] + 1) % 4 if out[pos] < 4 else 0
        elif what == "i":
            out.insert(pos, (out[pos] + 2) % 4 if out[pos] < 4 else 1)
        elif what == "d":
            del out[pos]
        elif what == "w":
            out[pos] = WILD
    return np.array(out, np.uint8)


class Planted:
    """a text, reads (or none: a self kind) and records of one sink kind"""

    def __init__(self, name, kind, text, palindromic=False):
        self.name, self.kind, self.palindromic = name, kind, palindromic
        self.text = np.asarray(text, np.uint8)
        self.reads, self.recs = [], []

    def add(self, p1, len1, v, distance, p2=None):
        """the record of text[p1 : p1 + len1] against v -- a read of its own
        (for a palindromic list: stored as its reverse complement) with two
        symbols around it, or (p2) text[p2 : p2 + len(v)] -- with the stored
        distance: > 0 edit operations, < 0 mismatches"""
        len2 = len(v)
        if self.kind in SELFKINDS:
            assert np.array_equal(self.text[p2:p2 + len2], v)
            seq2, start2 = p2, 0
        else:
            read = np.concatenate(([1, 2], v, [3])).astype(np.uint8)
            self.reads.append(rc(read) if self.palindromic else read)
            seq2, start2 = len(self.reads) - 1, 2
        if self.kind in (QUERY_EDIST, SELF_EDIST):
            length = len1 | distance << 48 | ((len2 - len1) & 0xFF) << 56
        elif self.kind in (QUERY_HAMMING, SELF_HAMMING):
            assert len1 == len2
            length = len1 | (-distance) << 48
        else:
            assert len1 == len2 and distance == 0
            length = len1
        self.recs.append((length, p1, seq2, start2))

    def records(self):
        rec = np.zeros(len(self.recs), H.MATCH_DTYPE)
        for i, x in enumerate(self.recs):
            rec[i] = x
        return rec

    def queries(self):
        return H.Queries.from_list(self.reads) if self.reads else None

    def triple(self):
        q = self.queries()
        return None if q is None else (q.symbols, q.start, q.length)

    def pairs(self, rec=None):
        q = self.queries()
        qt = None if q is None else (q.symbols, q.start, q.length,
                                     LETTERS[q.symbols])
        return [Pair(self.kind, x, self.palindromic, self.text,
                     LETTERS[self.text], [], qt)
                for x in (self.records() if rec is None else rec)]

    def model(self, rec=None):
        """-> (offsets, words)"""
        scripts = [p.script() for p in self.pairs(rec)]
        assert all(s is not None for s in scripts)
        return csr(scripts)


def _spread(n, d, rng):
    """d edits at least 9 symbols apart in a string of n symbols"""
    step = (n - 20) // d
    assert step >= 9
    return [(10 + i * step + int(rng.integers(0, step - 8)), "sid"[i % 3])
            for i in range(d)]


DISTANCES = (1, 7, 8, 15, 16, 31)   # 2 D + 1 = 15 | 17, 31 | 33: the widths


def planted_distance(D, palindromic=False):
    """records of stored distance D: the edits spread, only insertions
    (|ulen - vlen| = D: the end diagonal is the outermost lane), only
    deletions, an indel in the first and in the last column, a distance
    stored above the real one, a match at text position 0 and one that ends
    at the last symbol, a wildcard in either instance"""
    rng = np.random.default_rng(100 + D)
    n = 12 * D + 60
    text = rng.integers(0, 4, 3 * n + 50).astype(np.uint8)
    text[2 * n + 20] = WILD
    text[5 + n - 1] = (text[5 + n - 2] + 1) % 4   # a last column of its own
    sc = Planted("distance%d%s" % (D, "p" if palindromic else ""),
                 QUERY_EDIST, text, palindromic)
    u = text[5:5 + n]
    sc.add(5, n, edited(u, _spread(n, D, rng)), D)
    sc.add(5, n, edited(u, [(p, "i") for p, _ in _spread(n, D, rng)]), D)
    sc.add(5, n, edited(u, [(p, "d") for p, _ in _spread(n, D, rng)]), D)
    first = [(0, "i"), (n - 1, "d")] if D > 1 else [(0, "d")]
    sc.add(5, n, edited(u, first + [(p, "s") for p, _ in
                                    _spread(n, D - len(first), rng)]
                        if D > 2 else first), D)
    if D > 1:
        last = [(0, "d"), (n - 1, "i")]
        sc.add(5, n, edited(u, last), D)          # stored above the real one
    # the first and the last symbols of the text
    sc.add(0, n, edited(text[0:n], _spread(n, D, rng)), D)
    e = len(text)
    sc.add(e - n, n, edited(text[e - n:e], _spread(n, D, rng)), D)
    # a wildcard in the text / in the read (each costs an operation)
    w = 2 * n
    if D > 1:
        sc.add(w, n, edited(text[w:w + n], [(40, "s")]), D)
        sc.add(5, n, edited(u, [(33, "w")] + _spread(n, D - 1, rng)), D)
    return sc


def planted_tandem(kind=SELF_EDIST):
    """overlapping self matches: the two instances 1 .. 3 symbols apart in
    runs of one and of two symbols with an odd symbol inside (the same-text
    shortcut), or -- the same pairs as a palindromic query list -- in
    different arrays (no shortcut)"""
    rng = np.random.default_rng(7)
    text = rng.integers(0, 4, 400).astype(np.uint8)
    text[50:110] = 0
    text[80] = 2
    text[150:230] = np.tile([0, 3], 40)
    text[190] = 1
    text[300:360] = np.tile([1, 2, 3], 20)
    sc = Planted("tandem" if kind == SELF_EDIST else "tandem_as_queries",
                 kind, text, kind != SELF_EDIST)
    for p1, gap, n, d in ((55, 1, 40, 2), (56, 2, 44, 3), (60, 3, 40, 4),
                          (155, 2, 60, 2), (156, 1, 50, 3), (160, 3, 50, 4),
                          (302, 3, 40, 1), (303, 1, 45, 3), (304, 2, 45, 3)):
        # the largest distance the pair is within, for a stored one of d + 2
        p2 = p1 + gap
        sc.add(p1, n, text[p2:p2 + n], d + 2, p2)
    return sc


def planted_overshoot():
    """an insertion in front of symbols that agree with their neighbours:
    the backward slide passes the row the forward slide began at"""
    text = np.array([0, 1, 2, 3] * 5 + [2, 2, 2, 2, 2, 2] + [3, 1, 0, 2] * 5 +
                    [0, 0, 0, 0, 0] + [1, 3, 2, 0] * 4, np.uint8)
    sc = Planted("overshoot", QUERY_EDIST, text)
    n = len(text)
    for edits, d in (([(23, "i")], 1), ([(22, "d")], 1),
                     ([(23, "i"), (48, "d")], 2), ([(21, "i"), (50, "i")], 2)):
        v = edited(text, edits)
        # (the inserted symbol repeats the run it stands in)
        for pos, what in edits:
            if what == "i":
                v[pos] = text[pos]
        sc.add(0, n, v, d)
    return sc


def planted_longrun():
    """one identical run of more than 16383 symbols: a 40 000-symbol text
    whose second half repeats the first with one substitution"""
    rng = np.random.default_rng(11)
    half = rng.integers(0, 4, 20000).astype(np.uint8)
    other = half.copy()
    other[18000] = (other[18000] + 1) % 4
    text = np.concatenate((half, other))
    sc = Planted("longrun", SELF_EDIST, text)
    sc.add(0, 20000, other, 1, 20000)
    sc.add(10, 19000, text[20010:39010], 2, 20010)
    return sc


def planted_mixed(kind=QUERY_HAMMING, count=65):
    """`count` records of one list: exact ones and, by `kind`, -h or -e
    records of up to three substitutions; one of them 500 symbols longer"""
    rng = np.random.default_rng(13)
    text = rng.integers(0, 4, 700).astype(np.uint8)
    text[333] = WILD
    sc = Planted("mixed%d_%d" % (kind, count), kind, text)
    for i in range(count):
        n = 9 + 7 * (i % 9) + (500 if i == 3 else 0)
        p1 = (37 * i) % (len(text) - n)
        nd = i % 4 if kind != QUERY else 0
        places = sorted({int(x) for x in rng.integers(0, n, nd)})
        v = edited(text[p1:p1 + n], [(x, "s") for x in places])
        # (a wildcard in the window is one more difference of a record that
        # has any; a record of distance 0 is an identical run whatever it holds)
        dist = len(places) + (int((v >= WILD).sum()) if places else 0)
        sc.add(p1, n, v, dist if kind == QUERY_EDIST else -dist)
    return sc
