"""The recorded runs of vmatch -online -complete
(tests/golden/online_manifest.json, online_expected.npz, written by
scripts/make_golden_online.py): the recipes from which the vmatch command
line, the query files and the calls of the engine are derived, and the
hand-made texts for the edges of the scan.  Shared by the generator and the
two online test modules.

A run names a text -- a case of tests/golden/manifest.json, or a FASTA file
of tests/golden -- and its queries: the query file of the case, or reads
drawn from the text by a fixed-seed recipe (READS)."""
import hashlib
import json
import os

import numpy as np

import helpers as H
import online_model as OM

EXACT, EDIST, HAMMING = OM.EXACT, OM.EDIST, OM.HAMMING
SEP, WILD = H.SEPARATOR, H.WILDCARD


def R(key, text, reads, mode, K=0, percent=False, remred=False, strands="d"):
    return dict(key=key, text=text, reads=reads, mode=mode, K=K,
                percent=percent, remred=remred, strands=strands)


RUNS = [
    R("micro_exact", "micro", "file", EXACT),
    R("micro_h1", "micro", "file", HAMMING, 1),
    R("micro_h2", "micro", "file", HAMMING, 2),
    R("micro_e1", "micro", "file", EDIST, 1),
    R("micro_e2", "micro", "file", EDIST, 2),
    R("at1mb_e2", "at1mb", "mixed", EDIST, 2),
    R("at1mb_e3_remred", "at1mb", "mixed", EDIST, 3, remred=True),
    R("at1mb_h3", "at1mb", "mixed", HAMMING, 3),
    # 16 symbols: threshold 0 at 5 percent
    R("at1mb_e5p", "at1mb", "mixedshort", EDIST, 5, percent=True),
    R("at1mb_h10p", "at1mb", "mixedshort", HAMMING, 10, percent=True),
    # every window of 40 of the 52 symbols holds the seven wildcards of the
    # text, and up to 64 symbols a wildcard equals nothing: the reference
    # prints no line, which is what is recorded
    R("wildcards_e2", "wildcards", "wild4070", EDIST, 2),
    R("wildcards_h2", "wildcards", "wild4070", HAMMING, 2),
    R("tandem_e2_remred", "align_tandem.fna", "tandem", EDIST, 2, remred=True),
    R("tandem_e2", "align_tandem.fna", "tandem", EDIST, 2),
    R("micro_e1_dp", "micro", "file", EDIST, 1, strands="dp"),
    # shorter than the prefixlength of the index (6): the indexed exact search
    # refuses them
    R("grumbach_exact_short", "grumbach", "short", EXACT),
]


EMPTY = ("wildcards_e2",)   # runs without a line


def run_of(key):
    return next(r for r in RUNS if r["key"] == key)


def golden_keys():
    return [r["key"] for r in RUNS]


def vmatch_args(r):
    a = {"d": [], "p": ["-p"], "dp": ["-d", "-p"]}[r["strands"]]
    a += ["-online", "-complete"] + (["remred"] if r["remred"] else [])
    if r["mode"] != EXACT:
        a += ["-e" if r["mode"] == EDIST else "-h",
              "%d%s" % (r["K"], "p" if r["percent"] else "")]
    return a


# --------------------------------------------------------------------------
# texts and reads
# --------------------------------------------------------------------------

class Text:
    """tis, ssp (separator positions) of a run's text, the FASTA files it is
    made of and the prefixlength of its index"""

    def __init__(self, name):
        if name.endswith(".fna"):
            self.files = [name]
            self.tis, self.ssp, _ = H.fasta_text([os.path.join(H.GOLDEN,
                                                               name)])
            self.prefixlength = None
        else:
            m = H.manifest()[name]
            self.files = m["db"]
            idx, self.filequeries = H.load_case(name)
            self.tis, self.ssp = idx.tis, idx.ssp
            self.prefixlength = idx.prefixlength
        self.tis = np.ascontiguousarray(self.tis, np.uint8)
        self.ssp = np.asarray(self.ssp, np.uint64)
        self.n = len(self.tis)

    def seq_rel(self, pos):
        pos = np.asarray(pos, np.uint64)
        seq = np.searchsorted(self.ssp, pos, side="right").astype(np.uint64)
        starts = np.concatenate(([0], self.ssp + 1)).astype(np.uint64)
        return seq, pos - starts[seq]


_texts, _reads = {}, {}


def text_of(r):
    if r["text"] not in _texts:
        _texts[r["text"]] = Text(r["text"])
    return _texts[r["text"]]


def _edit(rng, q, subs=0, dele=0, ins=0):
    q = [int(c) for c in q]
    for _ in range(subs):
        x = int(rng.integers(2, len(q) - 2))
        if q[x] < 4:
            q[x] = (q[x] + 1 + int(rng.integers(0, 3))) % 4
    for _ in range(dele):
        del q[int(rng.integers(2, len(q) - 2))]
    for _ in range(ins):
        q.insert(int(rng.integers(2, len(q) - 2)), int(rng.integers(0, 4)))
    return q


def _window(t, rng, m, wild):
    """a window of m symbols of the text without a separator and with
    (`wild`) or without a wildcard, away from the low-complexity stretches"""
    for _ in range(100000):
        a = int(rng.integers(0, t.n - m))
        w = t.tis[a:a + m]
        if (w == SEP).any() or bool((w == WILD).any()) != wild:
            continue
        if wild and not (0 < int((w == WILD).sum()) <= 2):
            continue
        if len(set(w[:12].tolist())) < 4 or \
                max(np.bincount(w[w < 4], minlength=4)) > 0.45 * m:
            continue
        return a, w
    raise AssertionError("no window")


def _mixed(t, short):
    """reads of 32, 33, 64, 65 and 130 symbols (and 16 and 100), each a
    window of the text after a few edit operations; three of them carry a
    wildcard of the text, two of those beyond 64 symbols"""
    rng = np.random.default_rng(20240 + int(short))
    reads = []
    plan = [(32, 1, 0, 0, False), (33, 0, 1, 0, False), (64, 2, 0, 0, False),
            (65, 1, 0, 1, False), (130, 2, 1, 0, False), (100, 3, 0, 0, False),
            (40, 1, 0, 0, True), (70, 1, 0, 0, True), (130, 2, 0, 0, True)]
    if short:
        plan = [(16, 0, 0, 0, False)] + plan
    for m, s, d, i, wild in plan:
        _, w = _window(t, rng, m + d - i, wild)
        q = _edit(rng, w, s, d, i)
        assert len(q) == m
        reads.append(np.array(q, np.uint8))
    return reads


def _wild4070(t):
    """Wildcards.fna has 52 symbols: a window of 40 with its wildcards, and
    the whole text with 18 symbols of padding (70: it cannot match)"""
    assert t.n == 52
    a = t.tis[6:46].copy()
    b = np.concatenate((t.tis, np.tile([0, 1, 2, 3], 5)[:18])).astype(np.uint8)
    c = t.tis[2:42].copy()
    c[5] = (int(c[5]) + 1) % 4
    return [a, b, c]


def _tandem(t):
    """windows of the tandems of align_tandem.fna: whole runs of start
    positions"""
    tis = t.tis
    out = [tis[60:84].copy(), tis[100:130].copy(), tis[180:204].copy(),
           tis[262:287].copy()]
    for q in out:
        assert (q < 4).all()
    out[1][11] = (int(out[1][11]) + 1) % 4
    return out


def _short(t):
    """patterns of 3, 4 and 5 symbols of the text"""
    assert t.prefixlength == 6
    return [t.tis[1000:1005].copy(), t.tis[30000:30004].copy(),
            t.tis[50000:50005].copy(), t.tis[70000:70003].copy()]


def reads_of(r):
    """-> H.Queries of a run (direct strand)"""
    key = (r["text"], r["reads"])
    if key not in _reads:
        t = text_of(r)
        if r["reads"] == "file":
            q = t.filequeries
        else:
            make = {"mixed": lambda: _mixed(t, False),
                    "mixedshort": lambda: _mixed(t, True),
                    "wild4070": lambda: _wild4070(t),
                    "tandem": lambda: _tandem(t),
                    "short": lambda: _short(t)}[r["reads"]]
            q = H.Queries.from_list(make())
        _reads[key] = q
    return _reads[key]


def reads_fasta(q):
    """the reads as the text of a FASTA file (wildcards as n)"""
    chars = np.frombuffer(b"acgt", np.uint8)
    out = []
    for i in range(q.nq):
        s = q.seq(i)
        c = np.where(s < 4, chars[np.minimum(s, 3)], ord("n")).astype(np.uint8)
        out.append(">r%d\n%s\n" % (i, c.tobytes().decode()))
    return "".join(out)


def reverse_complement(q):
    sym = q.symbols.copy()
    for i in range(q.nq):
        s, l = int(q.start[i]), int(q.length[i])
        seg = q.symbols[s:s + l][::-1]
        sym[s:s + l] = np.where(seg >= WILD, seg, 3 - seg)
    return H.Queries(sym, q.start, q.length)


def passes(r):
    """[(palindromic, the batch of that pass)] in the order of the output"""
    q = reads_of(r)
    return ([(0, q)] if "d" in r["strands"] else []) + \
        ([(1, reverse_complement(q))] if "p" in r["strands"] else [])


def lists(q):
    return [q.seq(i) for i in range(q.nq)]


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


def rows_of(r, rec, palindromic):
    """records of the engine -> rows as vmatch prints them"""
    t, q = text_of(r), reads_of(r)
    rec = np.asarray(rec)
    out = np.zeros((len(rec), 8), np.int64)
    out[:, 0] = rec["length"]
    out[:, 1], out[:, 2] = t.seq_rel(rec["dbstart"])
    out[:, 3] = q.length.astype(np.int64)[rec["queryseq"].astype(np.int64)]
    out[:, 4] = rec["queryseq"]
    d = rec["querystart"].astype(np.int64)
    out[:, 6] = {EXACT: 0 * d, EDIST: d, HAMMING: -d}[r["mode"]]
    out[:, 7] = palindromic
    return out


def sink_kind(V, r):
    return {EXACT: V.SINK_COMPLETE, EDIST: V.SINK_APPROX_EDIST,
            HAMMING: V.SINK_APPROX_HAMMING}[r["mode"]]


def query_multiseq(q):
    length = q.length.astype(np.uint64)
    start = np.concatenate(([0], np.cumsum(length + np.uint64(1))[:-1]))
    return start.astype(np.uint64), length, int(length.sum()) + len(length) - 1


def sink_kwargs(V, r, palindromic):
    t, q = text_of(r), reads_of(r)
    kw = dict(kind=sink_kind(V, r), totallength=t.n, markpos=t.ssp,
              numofchars=4, palindromic=bool(palindromic))
    kw["querystart"], kw["querylength"], kw["querytotallength"] = \
        query_multiseq(q)
    return kw


def md5(text):
    return hashlib.md5(text).hexdigest()


_manifest = None
_arrays = None


def manifest():
    global _manifest
    if _manifest is None:
        with open(os.path.join(H.GOLDEN, "online_manifest.json")) as f:
            _manifest = json.load(f)
    return _manifest


def expected_rows(key):
    global _arrays
    if _arrays is None:
        _arrays = np.load(os.path.join(H.GOLDEN, "online_expected.npz"))
    return _arrays[key].astype(np.int64).reshape(-1, 8)


# --------------------------------------------------------------------------
# hand-made texts: the edges of the scan
# --------------------------------------------------------------------------

class Edge:
    """a text of a few thousand symbols and a batch of reads"""

    def __init__(self, name, text, reads):
        self.name = name
        self.text = np.ascontiguousarray(text, np.uint8)
        self.reads = [np.ascontiguousarray(q, np.uint8) for q in reads]

    def queries(self):
        return H.Queries.from_list(self.reads)


def _mutate(rng, w, k):
    q = w.copy()
    for x in rng.choice(np.arange(1, len(q) - 1), min(k, len(q) - 2),
                        replace=False) if len(q) > 2 and k else []:
        q[x] = (int(q[x]) + 1) % 4
    return q


def borders_edge(m, k, seed=1):
    """occurrences of one read that straddle the borders of tiles of 64, 256
    and the default, one at position 0 and one that ends at n; sequences
    shorter than m; a separator exactly on a tile border and m + k behind
    one.  2400 symbols, more for the long reads (whose occurrences are few:
    the model takes its time for each start position)"""
    n = 2400 if m <= 64 else 2400 + 3 * m if m <= 130 else 2000 + 5 * m
    rng = np.random.default_rng([seed, m, k])
    t = rng.integers(0, 4, n).astype(np.uint8)
    read = rng.integers(0, 4, m).astype(np.uint8)
    spots = [0, n - m]
    if m <= 64:
        for border in (64 * 9, 256 * 3, H_TILE * 4, 64 * 20):
            for off in (m // 2, 1, m - 1 if m > 1 else 0):
                spots.append(border - off)
    else:
        spots += [256 * 9 - m // 2, H_TILE * 12 - 1] if m > 130 else \
            [256 * 3 - m // 2, H_TILE * 4 - 1]
    for i, a in enumerate(sorted(set(spots))):
        assert 0 <= a and a + m <= n
        t[a:a + m] = _mutate(rng, read, i % (k + 1))
    # separators: on borders, m + k behind a border; two sequences shorter
    # than m
    for p in (64 * 13, 256 * 5, 256 * 6 + m + k, 64 * 30 + m + k):
        if p < n - m:
            t[p] = SEP
    if m > 2:
        a = 64 * 33 if m <= 130 else 64 * 41
        t[a] = SEP
        t[a + 1:a + m] = read[:m - 1]
        t[a + m] = SEP
        t[a + m + 1:a + m + m // 2 + 1] = read[:m // 2]
        t[a + m + m // 2 + 1] = SEP
    other = rng.integers(0, 4, m).astype(np.uint8)
    return Edge("borders_m%d_k%d" % (m, k), t, [read, other, read.copy()])


H_TILE = 296   # VSA_ONLINE_TILE_DEFAULT


def remred_edge(n=3000, seed=5):
    """runs of start positions: a tandem that crosses tile borders, and a
    read whose run holds a hit that does not improve (the dropped hit)"""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 4, n).astype(np.uint8)
    unit = np.array([0, 3], np.uint8)
    for a, reps in ((240, 20), (H_TILE * 2 - 30, 40), (64 * 19 - 9, 15)):
        t[a:a + 2 * reps] = np.tile(unit, reps)
    r0 = np.tile(unit, 10)
    r1 = rng.integers(0, 4, 30).astype(np.uint8)
    for a in (700, 1500, 2900):
        t[a:a + 30] = r1
    t[1500 + 11] = (int(t[1500 + 11]) + 1) % 4
    r2 = np.concatenate((r1[:15], r1[14:]))   # a symbol twice
    return Edge("remred", t, [r0, r1, r2])


def wildcard_edge(m, k, n=2000, seed=9):
    """wildcards in the text, in the pattern, and facing each other: copies
    of a read with 0, 1, 0 and 1 substitutions at 100, 600, 1100 and 1600;
    the second read carries a wildcard, which the copy at WILD_FACING faces
    with a wildcard of the text"""
    rng = np.random.default_rng([seed, m])
    t = rng.integers(0, 4, n).astype(np.uint8)
    read = rng.integers(0, 4, m).astype(np.uint8)
    wq = read.copy()
    wq[m // 3] = WILD
    for a, subs in ((100, 0), (600, 1), (1100, 0), (1600, 1)):
        t[a:a + m] = _mutate(rng, read, min(subs, k))
    t[WILD_FACING + m // 3] = WILD   # faces the wildcard of wq
    t[600 + m // 2] = WILD           # faces a regular symbol
    return Edge("wild_m%d_k%d" % (m, k), t, [read, wq])


WILD_FACING = 1100

LENGTHS = (1, 8, 31, 32, 33, 63, 64, 65, 128, 129, 512)


def thresholds(m):
    """0, 1, 3 and m / 10, below m"""
    return sorted({k for k in (0, 1, 3, m // 10) if k < m})


_model = {}


def model(edge, mode, K, percent=False, remred=False, offset=0):
    """the model's list of an edge, computed once"""
    key = (edge.name, mode, K, percent, remred)
    if key not in _model:
        _model[key] = OM.findcompletematches(edge.text, edge.reads, mode, K,
                                             percent, remred)
    out = _model[key].copy()
    out["queryseq"] += np.uint64(offset)
    return out
