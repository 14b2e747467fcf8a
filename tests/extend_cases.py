"""The recorded runs of vmatch -l L -h K outside -complete
(tests/golden/extend_manifest.json, extend_expected.npz, written by
scripts/make_golden_extend.py): the recipes from which the vmatch command
line, the seed lists and the calls of the engine are derived, and the
conversion between the rows vmatch prints and the records of the engine.
Shared by the generator and the two extend test modules."""
import hashlib
import json
import os

import numpy as np

import extend_model as EM
import helpers as H


def R(key, case, L, K, q=True, S=0, strands="d", alphabet=False, error=False):
    return dict(key=key, case=case, L=L, K=K, q=q, S=S, strands=strands,
                alphabet=alphabet, error=error)


# case: a case of tests/golden/manifest.json, or (alphabet) of
# alphabets_manifest.json.  q: with -q (seeds: MEMs), else the index against
# itself (seeds: maximal repeats).  strands "dp": -d -p, two passes.
RUNS = [
    R("c5_q_l40_h2", "c5", 40, 2),
    # -seedlength above L / (K + 1)
    R("c5_q_l40_h2_s20", "c5", 40, 2, S=20),
    # L / (K + 1) = 3 < prefixlength 6: the reference's error
    R("c5_q_l10_h2", "c5", 10, 2, error=True),
    R("at1mb_l60_h3", "at1mb", 60, 3, q=False),
    R("at1mb_l100_h8", "at1mb", 100, 8, q=False),
    R("grumbach_q_l30_h2_dp", "grumbach", 30, 2, strands="dp"),
    # (an index built with -db .. -q ..: database against query positions)
    R("grumbach_all_l30_h2", "grumbach_all", 30, 2, q=False),
    # a wildcard read gives matches of distance 1
    R("micro_q_l8_h1", "micro", 8, 1),
    R("wildcards_q_l8_h1", "wildcards", 8, 1),
    R("wildcards_l6_h2", "wildcards", 6, 2, q=False),
    R("prot_l12_h2", "prot", 12, 2, q=False, alphabet=True),
    R("prot_q_l12_h2", "prot", 12, 2, alphabet=True),
    # matches of thousands of symbols
    R("ychr3_l200_h20", "largepat", 200, 20, q=False),
]


def run_of(key):
    return next(r for r in RUNS if r["key"] == key)


def vmatch_args(r):
    a = {"d": [], "p": ["-p"], "dp": ["-d", "-p"]}[r["strands"]]
    a += ["-l", str(r["L"]), "-h", str(r["K"])]
    if r["S"]:
        a += ["-seedlength", str(r["S"])]
    return a


def load(r):
    """-> (Index, Queries or None)"""
    return (H.load_alphabet_case if r["alphabet"] else H.load_case)(r["case"])


def reverse_complement(q):
    """every sequence of the batch reversed and complemented in its place"""
    sym = q.symbols.copy()
    for i in range(q.nq):
        s, l = int(q.start[i]), int(q.length[i])
        seg = q.symbols[s:s + l][::-1]
        sym[s:s + l] = np.where(seg >= H.WILDCARD, seg, 3 - seg)
    return H.Queries(sym, q.start, q.length)


def passes(r):
    """the passes of a run in the order of the reference: [(palindromic,
    the batch the seeds are found in and extended in, or None)]"""
    idx, q = load(r)
    if not r["q"]:
        return [(0, None)]
    out = []
    if "d" in r["strands"]:
        out.append((0, q))
    if "p" in r["strands"]:
        out.append((1, reverse_complement(q)))
    return out


def seedlength(r):
    return EM.seedlength_rule(r["L"], r["K"], r["S"])


def oracle_seeds(r, queries):
    """the seed list of a pass from the CPU oracle, in reference order"""
    idx, _ = load(r)
    if queries is None:
        return H.oracle_repeats(idx, seedlength(r))
    return H.oracle_querymatches(idx, queries, seedlength(r), speedup=2)


def parse_rows(lines):
    """the default columns -> rows (length, seq1, rel1, seq2, rel2, distance,
    palindromic)"""
    out = np.zeros((len(lines), 7), np.int64)
    for i, l in enumerate(lines):
        f = l.split()
        assert f[0] == f[4]
        out[i] = (int(f[0]), int(f[1]), int(f[2]), int(f[5]), int(f[6]),
                  -int(f[7]), 1 if f[3] == "P" else 0)
    return out


def rows_of(r, rec, palindromic):
    """records of the engine -> rows as vmatch prints them"""
    idx, q = load(r)
    rec = np.asarray(rec)
    out = np.zeros((len(rec), 7), np.int64)
    length = EM.lengths(rec).astype(np.int64)
    out[:, 0] = length
    out[:, 1], out[:, 2] = idx.seq_rel(rec["dbstart"])
    out[:, 5] = EM.distances(rec)
    out[:, 6] = palindromic
    if r["q"]:
        out[:, 3] = rec["queryseq"]
        rel = rec["querystart"].astype(np.int64)
        if palindromic:
            qlen = q.length.astype(np.int64)[rec["queryseq"].astype(np.int64)]
            rel = qlen - (rel + length)
        out[:, 4] = rel
    else:
        s2, r2 = idx.seq_rel(rec["queryseq"])
        out[:, 3] = s2.astype(np.int64) - (idx.numofdbsequences
                                           if idx.hasqueries else 0)
        out[:, 4] = r2
    return out


def query_multiseq(q):
    """(start, length, total length) of the query Multiseq"""
    length = q.length.astype(np.uint64)
    start = np.concatenate(([0], np.cumsum(length + np.uint64(1))[:-1]))
    return start.astype(np.uint64), length, int(length.sum()) + len(length) - 1


def sink_kwargs(V, r, palindromic):
    """arguments of V.Sink for the lines of a pass"""
    idx, q = load(r)
    kw = dict(kind=V.SINK_QUERY_HAMMING if r["q"] else V.SINK_SELF_HAMMING,
              totallength=idx.n, markpos=idx.ssp, numofchars=idx.numofchars,
              leastlength=r["L"], palindromic=bool(palindromic))
    if r["q"]:
        kw["querystart"], kw["querylength"], kw["querytotallength"] = \
            query_multiseq(q)
    elif idx.hasqueries:
        kw["numofquerysequences"] = idx.numofsequences - idx.numofdbsequences
        kw["totalquerylength"] = idx.n - idx.querysepposition - 1
    return kw


def md5(text):
    return hashlib.md5(text).hexdigest()


_manifest = None
_arrays = None


def manifest():
    global _manifest
    if _manifest is None:
        with open(os.path.join(H.GOLDEN, "extend_manifest.json")) as f:
            _manifest = json.load(f)
    return _manifest


def expected_rows(key):
    global _arrays
    if _arrays is None:
        _arrays = np.load(os.path.join(H.GOLDEN, "extend_expected.npz"))
    return _arrays[key].astype(np.int64).reshape(-1, 7)


def golden_keys(error=False):
    return [r["key"] for r in RUNS if r["error"] == error]


# --------------------------------------------------------------------------
# seed lists made by hand: the border cases of the extension
# --------------------------------------------------------------------------

class Scenario:
    """A text, a batch of mutated copies of its windows (or none: seeds of
    the text against itself) and a list of seeds on exact stretches."""

    def __init__(self, name, n, rngseed, dense=False):
        self.name = name
        self.rng = np.random.default_rng(rngseed)
        self.text = self.rng.integers(0, 4, n).astype(np.uint8)
        self.reads, self.seeds, self.dense = [], [], dense
        self.params = []     # [(L, K, S)]

    def other(self, c):
        return (int(c) + 1 + int(self.rng.integers(0, 3))) % 4

    def read(self, w, m, mis=(), put=()):
        """a copy of text[w : w + m] with substitutions at the offsets `mis`
        and the symbols `put` = [(offset, symbol)] -> its number"""
        q = self.text[w:w + m].copy()
        q[q >= 4] = 0
        for o in mis:
            if 0 <= o < m:
                q[o] = self.other(q[o])
        for o, c in put:
            q[o] = c
        self.reads.append((w, q))
        return len(self.reads) - 1

    def seed(self, qi, o, s):
        """symbols [o, o + s) of read qi against their place in the text"""
        self.seeds.append((s, self.reads[qi][0] + o, qi, o))

    def planted(self, w, A, s, B, left=(), right=(), put=()):
        """a read of A + s + B symbols with a seed of s behind A: mismatches
        directly beside the seed and at the scan offsets left / right"""
        mis = [A - 1, A + s] + [A - 2 - t for t in left] + \
              [A + s + 1 + t for t in right]
        qi = self.read(w, A + s + B, mis, put)
        self.seed(qi, A, s)
        return qi

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
            m = len(self.reads[0][1])
            assert all(len(q) == m for _, q in self.reads)
            return H.Queries.uniform(np.concatenate([q for _, q in
                                                     self.reads]), m)
        return H.Queries.from_list([q for _, q in self.reads])

    def model(self, L, K, S):
        q = self.queries()
        return EM.extend(self.records(), self.text, 4, L, K, S,
                         None if q is None else (q.symbols, q.start,
                                                 q.length))


def _borders(dense):
    sc = Scenario("borders_dense" if dense else "borders", 700,
                  11 if dense else 12, dense)
    m, n = 64, 700
    if dense:
        # reads of one length back to back: no separator in memory
        for w in (0, 0, 130, 301, n - m, n - m):
            qi = sc.read(w, m, [9, 23, 31, 40, 57])
            for o in (0, 1, 2, 3, 10):
                sc.seed(qi, o, 6)
            for e in (m, m - 1, m - 2, m - 3, m - 12):
                sc.seed(qi, e - 6, 6)
        sc.params = [(12, 2, 0), (20, 5, 0), (8, 1, 0)]
        return sc
    # text positions 0, 1, 2 and the ends n - 1, n - 2, n - 3, in the first,
    # a middle and the last read of the batch
    for w, length in ((0, 80), (0, 41), (200, 57), (n - 80, 80), (n - 33, 33),
                      (1, 50), (n - 51, 50)):
        qi = sc.read(w, length, [7, 15, 22, 30, length - 9, length - 17])
        for o in (0, 1, 2, 3, 11):
            sc.seed(qi, o, 4)
        for e in (length, length - 1, length - 2, length - 3, length - 5):
            sc.seed(qi, e - 4, 4)
    # the text at its border, the read not: a read with symbols of its own
    # around the copy
    pre = sc.rng.integers(0, 4, 5).astype(np.uint8)
    q = np.concatenate((pre, sc.text[0:40], pre))
    sc.reads.append((-5, q))
    for o in (0, 1, 2, 3):
        sc.seeds.append((5, o, len(sc.reads) - 1, 5 + o))
    q = np.concatenate((pre, sc.text[n - 40:n], pre))
    sc.reads.append((n - 45, q))
    for e in (0, 1, 2, 3):
        sc.seeds.append((5, n - 5 - e, len(sc.reads) - 1, 40 - e))
    sc.params = [(10, 2, 0), (16, 5, 0), (6, 1, 0)]
    return sc


def _specials():
    """separators and wildcards beside the seed and within reach, in the
    text, in the read and facing each other"""
    sc = Scenario("specials", 1500, 13)
    t = sc.text
    for p in (100, 131, 260, 400, 433):
        t[p] = H.SEPARATOR
    for p in (600, 640, 700, 733, 790):
        t[p] = H.WILDCARD
    W = H.WILDCARD
    for sep in (100, 131, 260, 400, 433):
        for d in (1, 2, 3, 9, 17):
            # a seed of 8 that begins d behind / ends d in front of the
            # separator of the text
            sc.planted(sep + d - 20, 20, 8, 20, [3, 9], [4, 11])
            sc.planted(sep - d - 8 - 20, 20, 8, 20, [2, 7], [5])
    for wc in (600, 640, 700, 733, 790):
        for d in (1, 2, 3, 9, 17):
            sc.planted(wc + d - 20, 20, 8, 20, [6], [7])
            sc.planted(wc - d - 8 - 20, 20, 8, 20, [6], [7])
    for d in (1, 2, 3, 9, 17):
        # a wildcard of the read, and two wildcards facing each other
        sc.planted(900, 30, 8, 30, [12], [13], [(30 - d, W), (38 + d - 1, W)])
        sc.planted(670 + d, 30, 8, 30, [11], [14], [(30 - d, W)])
        sc.planted(663 - d, 30, 8, 30, [11], [14], [(37 + d, W)])
    sc.params = [(14, 2, 0), (24, 5, 0), (10, 1, 0)]
    return sc


def _alignment():
    """every combination of dbstart % 8 and querystart % 8 in memory, the
    mismatches some ten symbols apart"""
    sc = Scenario("alignment", 4000, 14)
    start = 0
    for i in range(8):
        w = 160 + (start + i) % 8
        m = 420 + 3 * i
        mis = list(np.cumsum(sc.rng.integers(6, 19, 60)))
        mis = [x for x in mis if x < m and not 200 <= x < 212]
        qi = sc.read(w + 300 * i, m, mis)
        for o in range(200, 208):
            sc.seed(qi, o, 4)
        start += m + 1
    sc.params = [(30, 2, 0), (60, 5, 0), (12, 1, 0), (200, 64, 0),
                 (40, 5, 3000)]
    return sc


def alignment_residues(sc):
    q = sc.queries()
    return {(int(d) % 8, (int(q.start[int(qi)]) + int(o)) % 8)
            for _, d, qi, o in sc.seeds}


def _offsets(name, places, context, rngseed):
    """the mismatch that ends a scan at the scan offsets `places`, on the
    left and on the right; K = 2: two mismatches in front of it.  (The text
    is short; the batch of its long copies is what grows with `context`.)"""
    sc = Scenario(name, 2 * context + 200, rngseed)
    for T in places:
        sc.planted(50, context + 10, 12, 10, [2, 5, T], [3])
        sc.planted(50 + context, 10, 12, context + 10, [3], [2, 5, T])
        # ... and nothing but that one mismatch
        sc.planted(50, context + 10, 12, 10, [T], [])
        sc.planted(50 + context, 10, 12, context + 10, [], [T])
    # (with a seed length nothing reaches, the left stop rule is out of the
    # way; without, it ends the left scans early)
    sc.params = [(30, 2, 100000), (30, 2, 0), (30, 1, 100000), (30, 5, 100000)]
    return sc


def _stoprule():
    """exact stretches of seedlength and seedlength + 1 between two
    mismatches on the left, where the scan stops behind the longer one, and
    on the right, where it does not; L = 60, K = 2: seedlength 20"""
    sc = Scenario("stoprule", 900, 17)
    for first in (0, 4, 9):
        for gap in (19, 20, 21, 22):
            # look[h] - look[h - 1] = gap
            sc.planted(100, 120, 20, 120, [first, first + gap,
                                           first + gap + 7], [])
            sc.planted(100, 120, 20, 120, [], [first, first + gap,
                                               first + gap + 7])
            sc.planted(400, 120, 20, 120, [first, first + gap],
                       [first, first + gap])
    sc.params = [(60, 2, 0), (60, 5, 0), (60, 2, 21), (40, 1, 0)]
    return sc


def _fewmismatches():
    """hleft + hright < K: short sides that end at the borders of the reads;
    seeds as long as L and longer; a long match whose E-values are all 0.0"""
    sc = Scenario("fewmismatches", 2600, 18)
    for A, B in ((0, 0), (1, 1), (2, 2), (3, 9), (9, 3), (12, 12), (0, 14)):
        sc.planted(300 + A, A, 30, B, [4] if A > 8 else [],
                   [5] if B > 8 else [])
    for s in (40, 41, 60):
        sc.planted(500, 25, s, 25, [3, 12], [2, 9, 17])
    # more than 600 symbols with few mismatches: identity and length decide
    sc.planted(1000, 400, 30, 420, [100, 250, 390], [120, 300, 410])
    sc.planted(1000, 400, 30, 420, [390], [])
    sc.planted(1700, 320, 25, 330, [], [40, 300])
    sc.params = [(40, 5, 0), (40, 2, 0), (30, 1, 0), (700, 5, 0), (40, 64, 0)]
    return sc


def _selfseeds():
    """seeds of a text against itself: planted repeats with mismatches,
    separators and the borders of the text"""
    sc = Scenario("selfseeds", 3000, 19)
    t = sc.text
    t[1500] = H.SEPARATOR
    for a, b, m in ((0, 1501, 300), (400, 2000, 350), (800, 2600, 400),
                    (1150, 2380, 200)):
        m = min(m, len(t) - b, 1500 - a)
        t[b:b + m] = t[a:a + m]
        for x in np.cumsum(sc.rng.integers(5, 40, 30)):
            if x < m:
                t[b + x] = sc.other(t[b + x])
        for o in range(0, m - 12, 7):
            if np.array_equal(t[a + o:a + o + 8], t[b + o:b + o + 8]):
                sc.selfseed(a + o, b + o, 8)
    t[2000 + 170] = H.WILDCARD
    t[400 + 171] = H.WILDCARD
    sc.params = [(30, 2, 0), (40, 5, 0), (16, 1, 0), (60, 64, 0)]
    return sc


def scenarios(lane_budget, long_step):
    """name -> Scenario; the two limits are those the library exports"""
    near = [7, 8, 9, 15, 16, 17]
    out = [
        _borders(False), _borders(True), _specials(), _alignment(),
        _offsets("budget", near + [lane_budget - 9, lane_budget - 8,
                                   lane_budget - 1, lane_budget,
                                   lane_budget + 1, lane_budget + 7,
                                   lane_budget + 8], lane_budget + 40, 15),
        _offsets("longstep", [long_step - 17, long_step - 16, long_step - 1,
                              long_step, long_step + 1, long_step + 15,
                              long_step + 16], long_step + 60, 16),
        _stoprule(), _fewmismatches(), _selfseeds(),
    ]
    return {sc.name: sc for sc in out}


SCENARIOS = ("borders", "borders_dense", "specials", "alignment", "budget",
             "longstep", "stoprule", "fewmismatches", "selfseeds")
