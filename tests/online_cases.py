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

# low-complexity texts: every position a hit, runs of start positions as long
# as a sequence; the period-3 text has four sequences
for _name, _runs in (("homopolymer", "h1 e1 e1r e3 e3r"),
                     ("period2", "h1 e1 e1r e3 e3r"),
                     ("period3", "e1r e3r")):
    for _w in _runs.split():
        RUNS.append(R("%s_%s%s" % (_name, _w[:2], "_remred" * (len(_w) > 2)),
                      "online_%s.fna" % _name, _name,
                      EDIST if _w[0] == "e" else HAMMING, int(_w[1]),
                      remred=len(_w) > 2))
# texts of 7, 8 and 9 symbols with reads of n to n + 3 symbols: a staged word
# that ends in the padding, reads longer than the text
for _n in (7, 8, 9):
    for _w, _mode, _k in (("exact", EXACT, 0), ("h1", HAMMING, 1),
                          ("e1", EDIST, 1), ("e2", EDIST, 2)):
        RUNS.append(R("tiny%d_%s" % (_n, _w), "online_tiny%d.fna" % _n,
                      "tiny", _mode, _k))


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


def _periodic(unit, lengths):
    sym = np.array(["acgt".index(c) for c in unit], np.uint8)
    return [np.tile(sym, m // len(sym) + 1)[:m] for m in lengths]


def _tiny(t):
    """the text and 0 to 3 more symbols"""
    more = np.array([0, 1, 2], np.uint8)
    return [np.concatenate((t.tis, more[:i])) for i in range(4)]


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
                    "short": lambda: _short(t),
                    "homopolymer": lambda: _periodic("a", (4, 9, 33, 70)),
                    "period2": lambda: [_periodic("at", (4,))[0],
                                        _periodic("ta", (9,))[0]] +
                    _periodic("at", (34, 80)),
                    "period3": lambda: [_periodic("acg", (6,))[0],
                                        _periodic("cga", (10,))[0],
                                        _periodic("acg", (66,))[0]],
                    "tiny": lambda: _tiny(t)}[r["reads"]]
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


# --------------------------------------------------------------------------
# the edges of the driver: workgroups of the edit scan, groups and chunks of
# queries, dense hits, tiny texts.  An Edge here carries the thresholds it is
# made for (Ks: (K, percent) pairs) and what it planted.
# --------------------------------------------------------------------------

WG_TILES = 128    # tiles a workgroup of the edit scan stages (ON_BLOCK)
GROUP = 32        # queries a workgroup loops over (ON_GROUP)
WTILE = 2048      # start positions of a tile of the window scans (ON_WTILE)
MODES = ((EXACT, False), (HAMMING, False), (EDIST, False), (EDIST, True))

WG_SIZES = {64: (8191, 8192, 8193, 8192 + 67, 2 * 8192 + 5),
            None: (H_TILE * WG_TILES + 600,)}
WG_LENGTHS = (8, 33, 65)
WG_K = 2


def wg_edge(tile, n, sep=0):
    """a random text of n symbols around the border of the first workgroup of
    the edit scan with tiles of `tile` symbols (border = 128 tiles); reads of
    8, 33 and 65 symbols.  Each read is a window of the text that straddles
    the border -- its start at border - m / 2, border - 1, border - m + 1 or
    on the border, which of them turns with n -- or, where the text ends at
    the border, the window that ends with the text or one symbol behind the
    border.  Copies with 0 to 2 substitutions: at a second border where the
    text has one, at n - m for one read and in front of that for the others
    (the last tiles), and a copy of the 33-symbol read without one symbol
    (-e alone finds it).  sep == 1: a separator at border - 1, a copy of one
    read that starts on the border and a separator m + k behind the border;
    sep == 2: the same one symbol further to the right (the separator on the
    border)."""
    T = tile or H_TILE
    b = T * WG_TILES
    rng = np.random.default_rng([77, T, n, sep])
    t = rng.integers(0, 4, n).astype(np.uint8)
    rot = (n + sep) % 4
    reads, starts = [], []
    for i, m in enumerate(WG_LENGTHS):
        off = (m // 2, 1, m - 1, 0)[(i + rot) % 4]
        if b - off + m > n:
            off = m - 1 if b + 1 <= n else b - (n - m)
        starts.append(b - off)
        reads.append(t[b - off:b - off + m].copy())
        assert len(reads[-1]) == m
    if 2 * b + 66 <= n:
        # the second border: the same windows, one symbol of each changed
        t[2 * b - 65:2 * b + 66] = t[b - 65:b + 66]
        for x in (2 * b - 3, 2 * b + 2):
            t[x] = (int(t[x]) + 1) % 4
    # the end of the text and the last tiles, where that is not the border
    a, first = n, rot % 3
    if n >= b + 66 + sum(WG_LENGTHS) + 9:
        for j, i in enumerate([first] + [i for i in range(3) if i != first]):
            m = WG_LENGTHS[i]
            a -= m
            t[a:a + m] = _mutate(rng, reads[i], j % (WG_K + 1))
            a -= 3
    # a deletion, in the middle of the first workgroup
    x = b // 2 - 11
    t[x:x + 32] = np.delete(reads[1], 16)
    planted = dict(border=b, starts=starts, indel=x)
    if sep:
        s = b - 2 + sep
        for i in ((rot + 1) % 3, 1, 0):
            m = WG_LENGTHS[i]
            if s + 1 + m + WG_K + 1 < min(n, a):
                t[s + 1:s + 1 + m] = reads[i]
                t[s + 1 + m + WG_K] = SEP
                planted["onborder"] = (i, s + 1)
                break
        t[s] = SEP
    e = Edge("wg_t%d_n%d_s%d" % (T, n, sep), t, reads)
    e.Ks, e.planted = [(WG_K, False)], planted
    return e


def wg_edges(tile):
    out = [wg_edge(tile, n) for n in WG_SIZES[tile]]
    big = WG_SIZES[tile][-2] if tile else WG_SIZES[tile][0]
    return out + [wg_edge(tile, big, 1), wg_edge(tile, big, 2)]


GROUP_LENGTHS = (1, 2, 7, 8, 9, 12, 31, 32, 33, 63, 64, 65, 100, 129, 257,
                 300)
GROUP_NQ = (31, 32, 33, 65, 97)
GROUP_EMPTY, GROUP_WILD40, GROUP_WILD70 = 17, 5, 13   # reads with a role
GROUP_K0 = (1, True)    # threshold 0 for every read but the longest


def _absent(m):
    """a read that occurs nowhere in a text without the symbol 3"""
    return np.full(m, 3, np.uint8)


def groups_edge(nq, longest=300, hitters=None):
    """a text of 3000 symbols over three of the four symbols, with the
    fourth in what is planted only, and nq reads whose lengths cycle through
    GROUP_LENGTHS (the last of them `longest`: 300, or 512).  Reads 0, 31, 32
    and nq - 1 are windows of the text with a substitution each beyond 12
    symbols; the others are random, so the short ones hit often and the long
    ones never; with 97 reads the third group of 32 (reads 64 to 95) holds
    reads of the absent symbol only and hits nowhere.  Read GROUP_EMPTY has
    no symbol.  Reads GROUP_WILD40 and GROUP_WILD70 (40 and 70 symbols) carry
    a wildcard that faces a wildcard of the text, as in wildcard_edge.
    hitters: the reads that may hit at all (windows of the text); every other
    read is of the absent symbol."""
    n = 3000
    rng = np.random.default_rng([31, nq, longest, len(hitters or ())])
    t = rng.integers(0, 3, n).astype(np.uint8)
    lengths = [longest if m == 300 else m
               for m in (GROUP_LENGTHS * 7)[:nq]]
    planted = tuple(sorted({0, 31, 32, nq - 1} & set(range(nq)))) \
        if hitters is None else tuple(hitters)
    silent = range(64, 96) if hitters is None and nq >= 96 else ()
    facing, wild = {}, {}
    if hitters is None:
        for i, m, a in ((GROUP_WILD40, 40, 700), (GROUP_WILD70, 70, 1900)):
            t[a + m // 3] = WILD
            wild[i] = t[a:a + m].copy()
            facing[i] = a
    reads = []
    for i, m in enumerate(lengths):
        if i in planted:
            q = np.array([WILD], np.uint8)
            while (q == WILD).any():
                a = int(rng.integers(0, n - m))
                q = t[a:a + m].copy()
            if m > 12:
                q[m // 2] = 3
        elif i in silent or hitters is not None:
            q = _absent(m)
        else:
            q = rng.integers(0, 4 if m > 2 else 3, m).astype(np.uint8)
        reads.append(q)
    if hitters is None:
        reads[GROUP_EMPTY] = np.zeros(0, np.uint8)
        for i, q in wild.items():
            reads[i] = q
    e = Edge("groups_%d_%d_%s" % (nq, longest, "all" if hitters is None else
                                  "-".join(map(str, planted))), t, reads)
    e.Ks = [(5, True), (10, True), (20, True)]
    e.planted = dict(planted=planted, silent=tuple(silent), facing=facing)
    return e


def uniform_edge(nq, m=41, hitters=None):
    """nq reads of one length that is no multiple of 4, for the batch forms
    whose symbol addressing multiplies by the absolute query number: a text
    of 3000 symbols; every third read (or `hitters`) is a window of the text
    with one substitution, the others are random; read 1 carries a wildcard
    facing one of the text (a packed batch keeps it in its side list)."""
    n = 3000
    rng = np.random.default_rng([41, nq, m, len(hitters or ())])
    t = rng.integers(0, 4, n).astype(np.uint8)
    hit = set(range(0, nq, 3)) | {nq - 1} if hitters is None else set(hitters)
    reads = []
    for i in range(nq):
        q = rng.integers(0, 4, m).astype(np.uint8)
        if i in hit:
            a = int(rng.integers(0, n - m))
            q = t[a:a + m].copy()
            q[m // 2] = (int(q[m // 2]) + 1) % 4
        reads.append(q)
    a = 1234
    t[a:a + m] = reads[1]
    t[a + m // 3] = reads[1][m // 3] = WILD
    e = Edge("uniform_%d_%d_%s" % (nq, m, "third" if hitters is None else
                                   "-".join(map(str, sorted(hit)))), t, reads)
    e.Ks = [(2, False)]
    e.planted = dict(planted=tuple(sorted(hit)))
    return e


DENSE_KINDS = ("homopolymer", "period2", "period3sep")
DENSE_SIZES = (2047, 2048, 2049, 4200)
DENSE_KS = ((1, True), (1, False), (3, False))   # 1 percent: threshold 0


def dense_edge(kind, n):
    """low-complexity text: a homopolymer, a text of period 2, one of period
    3 with a separator every 701 symbols; reads of 4, 9, 33 and 66 symbols of
    the same period and one out of phase (a foreign symbol for the
    homopolymer)."""
    unit = {"homopolymer": [0], "period2": [0, 3],
            "period3sep": [0, 1, 2]}[kind]
    p = len(unit)
    t = np.tile(np.array(unit, np.uint8), n // p + 1)[:n]
    if kind == "period3sep":
        t[700::701] = SEP
    reads = [np.tile(np.array(unit, np.uint8), m // p + 1)[:m]
             for m in (4, 9, 33, 66)]
    if p == 1:
        reads.append(np.full(4, 1, np.uint8))
    else:
        reads.append(np.tile(np.array(unit[1:] + unit[:1], np.uint8), 5))
    e = Edge("dense_%s_%d" % (kind, n), t, reads)
    e.Ks, e.planted = list(DENSE_KS), {}
    return e


TINY_SIZES = (1, 2, 3, 7, 8, 9, 63, 64, 65)
# a read of one symbol is in the batch: -e on the device takes thresholds
# below 1 for it, i.e. K = 0 or a percentage.  50 percent of 2, 4 and 8
# symbols is 1, 2 and 4.
TINY_KS = ((0, False), (20, True), (50, True))


def tiny_edge(n, sep=False):
    """a text of n symbols; reads: the text, the text and 1 and 3 more
    symbols, the text without its last symbol (not for n = 1), one foreign
    symbol.  sep: a separator in the middle of the text (the reads keep the
    symbol it replaces)."""
    rng = np.random.default_rng([11, n])
    t = rng.integers(0, 3, n).astype(np.uint8)
    more = rng.integers(0, 3, 3).astype(np.uint8)
    reads = [t.copy(), np.concatenate((t, more[:1])), np.concatenate((t, more))]
    if n > 1:
        reads.append(t[:-1].copy())
    reads.append(_absent(1))
    if sep:
        t[n // 2] = SEP
    e = Edge("tiny_%d_%d" % (n, int(sep)), t, reads)
    e.Ks, e.planted = list(TINY_KS), {}
    return e


def empty_edges():
    """the empty text with reads, and a text with an empty batch"""
    a = Edge("tiny_0", np.zeros(0, np.uint8), tiny_edge(3).reads)
    b = Edge("tiny_noreads", tiny_edge(9).text, [])
    a.Ks = b.Ks = [(0, False), (50, True)]
    return [a, b]


def modes_of(edge, K, percent, device=True):
    """the (mode, remred) pairs a threshold goes with: a fixed K above 0
    says nothing new for exact; -e on the device refuses a threshold that is
    not below every read"""
    out = []
    for mode, remred in MODES:
        if mode == EXACT and (percent or K != edge.Ks[0][0]) and \
                (K, percent) != edge.Ks[0]:
            continue
        if mode == EDIST and device and edge.reads and \
                (K >= 100 if percent else
                 K >= min(len(q) for q in edge.reads)):
            continue
        out.append((mode, remred))
    return out


def edge_model(edge, mode, K, percent=False, remred=False, offset=0):
    """model() with the list left unchanged for the next test"""
    return model(edge, mode, K, percent, remred, offset)


def expected_stats(edge, mode, K, percent, tile):
    """(candidates, searches) the device must report: the start positions
    before remred, and the distinct (query, tile) pairs they lie in -- tiles
    of `tile` symbols for -e, of WTILE start positions otherwise"""
    plain = model(edge, mode, K, percent, False)
    T = (tile or H_TILE) if mode == EDIST else WTILE
    pairs = set(zip(plain["queryseq"].tolist(),
                    (plain["dbstart"] // np.uint64(T)).tolist()))
    return len(plain), len(pairs)


def setcounters(monkeypatch, counters):
    if counters is None:
        monkeypatch.delenv("VSA_ONLINE_COUNTERS", raising=False)
    else:
        monkeypatch.setenv("VSA_ONLINE_COUNTERS", str(counters))
