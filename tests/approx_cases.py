"""Seeded cases for approximate complete matches at the structural edges of
the kernels (approx_search.inc, approx_device.hpp), shared by the CPU test of
the model (test_approx_model_host.py) and the GPU test
(test_gpu_approx_edges.py).

Texts: three sequences joined by separators, the first starting at text
position 0 and the last ending at n - 1, a few wildcards away from the
borders, the head of the first sequence planted again (two substitutions) at
the very end of the last one.  Reads hold no special symbol.

A case is one batch of reads with one threshold rule.  GROUPS names the
lists of one-length cases the tests are parametrised by; mixed_cases,
plan_cases, hits_case, last_read_case and too_long_reads build the others;
expected(case) is the oracle's list and the model's set, computed once.
"""
import numpy as np

import helpers as H

LENGTHS = [63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 321,
           383, 384, 385, 448, 449, 511, 512]
# 8t - 1, 8t, 8t + 1 around 96 and 152: the band takes rows eight at a time
BAND_LENGTHS = [95, 96, 97, 151, 152, 153]
TABLE_READS = 4096   # apm_plan: more reads than this of mixed lengths (none
                     # beyond VSA_APM_TABLEMAX = 4096 symbols) are planned
                     # through per-length tables filled on the device


class Case:
    def __init__(self, name, text, reads, doedist, k, percent=0, uniform=False,
                 words=None, border=False, hits=None, note=""):
        self.name, self.text, self.reads = name, text, reads
        self.doedist, self.k, self.percent = doedist, k, percent
        self.uniform = uniform      # one length: also runs as a packed batch
        self.words = words          # W of ApmColumn<W> in the region scan
        self.border = border        # must hold matches flush to both borders
        self.hits = hits            # piece hits: (of the marked read, in all)
        self.note = note

    def thresholds(self):
        m = np.array([len(r) for r in self.reads])
        return m * self.k // 100 if self.percent else np.full(len(m), self.k)

    def queries(self):
        """the batch as bytes: one length -> read i at i * m, nothing between
        the reads; several lengths -> separators between the reads, nothing
        behind the last one"""
        if self.uniform:
            return H.Queries.uniform(np.concatenate(self.reads),
                                     len(self.reads[0]))
        return H.Queries.from_list(self.reads)


_texts = {}


def text(which="long"):
    """long: sequences of 1187, 1403 and 1291 symbols (reads of 512 symbols
    from both ends of each leave room for wildcards in the middle); short:
    701, 1013, 857"""
    if which not in _texts:
        rng = np.random.default_rng(7 if which == "long" else 11)
        lens = (1187, 1403, 1291) if which == "long" else (701, 1013, 857)
        clear = 520 if which == "long" else 160   # no wildcard this close
        seqs = []
        for L in lens:
            s = rng.integers(0, 4, L).astype(np.uint8)
            s[rng.integers(clear, L - clear, 3)] = H.WILDCARD
            seqs.append(s)
        head = seqs[0][:clear - 20].copy()        # (holds no wildcard)
        for x in (47, 111):
            head[x] = (head[x] + 1) % 4
        seqs[2][-len(head):] = head
        tis = np.concatenate([np.concatenate([s, [H.SEPARATOR]])
                              for s in seqs])[:-1].astype(np.uint8)
        assert tis[0] < 4 and tis[-1] < 4
        _texts[which] = (tis, clear)
    return _texts[which][0]


def sequences(tis):
    """[(first position, length)] of the sequences of a text"""
    b = np.concatenate([[-1], np.flatnonzero(tis == H.SEPARATOR), [len(tis)]])
    return [(int(a) + 1, int(c - a - 1)) for a, c in zip(b[:-1], b[1:])]


def _edited(seq, m, end, flush, ops, rng):
    """a read of exactly m symbols cut from seq at distance `flush` (0 or 1)
    from its first (end = 0) or last (end = 1) symbol, after the edit
    operations ops = [(kind, where)]: kind 0 substitution, 1 a symbol of the
    text missing in the read, 2 a symbol more in the read; where 0 on the
    first read symbol, 1 on the last, 2 somewhere inside"""
    need = m + sum(k == 1 for k, _ in ops) - sum(k == 2 for k, _ in ops)
    a = flush if end == 0 else len(seq) - need - flush
    q = [int(c) for c in seq[a:a + need]]
    assert len(q) == need and max(q) < 4, "a wildcard near a border"
    inside = list(rng.choice(np.arange(8, m - 8), len(ops), replace=False))
    for kind, where in ops:
        x = 0 if where == 0 else (len(q) - 1 if where == 1 else int(inside.pop()))
        if kind == 0:
            q[x] = (q[x] + 1 + int(rng.integers(0, 3))) % 4
        elif kind == 1:
            del q[x]
        else:
            q.insert(x + (where == 1), (q[x] + 1 + int(rng.integers(0, 3))) % 4)
    assert len(q) == m
    return np.array(q, np.uint8)


_border = {}


def border_reads(which, m, k, doedist):
    """for every sequence of the text: reads cut at offsets 0, 1, L - m - 1
    and L - m (before the edits), each with 0, 1 and k edit operations
    (substitutions only for Hamming distance); operations fall on the first
    and on the last read symbol in turn, so that the best alignment wants to
    leave the sequence"""
    key = (which, m, k, doedist)
    if key in _border:
        return _border[key]
    tis = text(which)
    rng = np.random.default_rng([m, k, int(doedist)])
    # which operation falls where changes from read to read and, through m,
    # from length to length: a lone operation goes through all nine pairs of
    # (kind, place), the operations on the first and on the last symbol of a
    # read with K of them through all nine pairs of kinds
    reads, one, many = [], m, m
    for a, L in sequences(tis):
        seq = tis[a:a + L]
        for end in (0, 1):
            for flush in (0, 1):
                for nops in sorted({0, 1, k}):
                    if nops == 0:
                        ops = []
                    elif nops == 1:
                        ops = [((one // 3) % 3, one % 3)]
                        one += 1
                    else:
                        kinds = [many % 3, (many // 3) % 3] + \
                            [(many + i) % 3 for i in range(nops - 2)]
                        ops = list(zip(kinds, [0, 1] + [2] * (nops - 2)))
                        many += 1
                    if not doedist:
                        ops = [(0, w) for _, w in ops]
                    reads.append(_edited(seq, m, end, flush, ops, rng))
    _border[key] = reads
    return reads


def band_k(m):
    # (1, 2, 3), (2, 3, 1), (3, 1, 2) over the triples 64 w - 1, 64 w, 64 w + 1
    i = (LENGTHS + BAND_LENGTHS).index(m)
    return 1 + (i + i // 3) % 3


def scan_k(m):
    return 4 + LENGTHS.index(m) % 2


def words(m):
    return (m + 63) // 64


def _which(m):
    return "long" if m > 160 else "short"


def uniform_case(kind, m):
    """one length, the border reads: kind band (edit distance, K <= 3; runs
    through the banded alignment and, forced, through the region scan), scan
    (edit distance, K = 4 | 5: the region scan, ApmColumn<words(m)>), hamming"""
    doedist = kind != "hamming"
    k = scan_k(m) if kind == "scan" else band_k(m)
    return Case("%s_m%d_k%d" % (kind, m, k), text(_which(m)),
                border_reads(_which(m), m, k, doedist), doedist, k,
                uniform=True, words=words(m), border=True,
                note="W = %d" % words(m))


def mixed_case(kind, longest, k, percent=0, copies=None):
    """reads of every listed length up to `longest` in one batch -- the
    longest read fixes W for all (W = 8 for 512, W = 6 for 384), the shorter
    ones end their columns in an earlier word; three reads of each length,
    short and long ones interleaved, a short read last.  percent: K percent
    of the length, so that reads have thresholds of their own below the
    batch's largest.  copies: the batch repeated cyclically to that many
    reads (the three forms of the plan)"""
    doedist = kind != "hamming"
    lens = [m for m in LENGTHS if m <= longest and
            (not percent or 1 <= m * k // 100)]
    reads = []
    for i, m in enumerate(lens):
        kk = m * k // 100 if percent else k
        pool = border_reads("long", m, kk, doedist)
        reads += [pool[(5 * i + 7 * j) % len(pool)] for j in range(3)]
    order = np.random.default_rng(longest + k).permutation(len(reads))
    reads = [reads[i] for i in order]
    reads.sort(key=lambda r: len(r) == lens[0])    # stable: the shortest last
    assert len(reads[-1]) == lens[0] and max(map(len, reads)) == longest
    if copies:
        reads = [reads[i % len(reads)] for i in range(copies)]
    name = "mixed_%s_to%d_%s%d%s%s" % (kind, longest, "e" if doedist else "h",
                                       k, "p" if percent else "",
                                       "_x%d" % copies if copies else "")
    return Case(name, text("long"), reads, doedist, k, percent,
                words=words(longest), note="W = %d" % words(longest))


def piece_hits(tis, n_for_split, read, doedist, k):
    """how often the pieces of a read occur in the text: the pieces of
    realsplitesaapm (offsets 0, splitlen, .. while a whole piece fits),
    counted symbol by symbol"""
    m = len(read)
    size = int(H.oracle_lib().orc_getoptsplit(int(doedist), 10, 4,
                                              n_for_split, m, k))
    sl = m // size
    win = np.lib.stride_tricks.sliding_window_view(tis, sl)
    return sum(int((win == read[o:o + sl]).all(axis=1).sum())
               for o in range(0, m - sl + 1, sl))


def hits_case(kind, target):
    """one read whose two pieces of 32 symbols occur `target` times in all:
    the whole read planted target // 2 times, its first piece once more for
    an odd target.  VSA_APM_SEGMAX = 64 hits of one read is where the sort
    inside the reads hands over to the radix sort of the batch.  Around it a
    few ordinary reads; the marked read is the second of the batch."""
    doedist = kind != "hamming"
    rng = np.random.default_rng(target)
    seqs = [rng.integers(0, 4, 3000).astype(np.uint8) for _ in range(3)]
    read = rng.integers(0, 4, 64).astype(np.uint8)
    spots = [(s, x) for s in (1, 2, 0) for x in range(40, 2900, 70)]
    for s, x in spots[:target // 2]:
        seqs[s][x:x + 64] = read
    if target % 2:
        s, x = spots[target // 2]
        seqs[s][x:x + 32] = read[:32]
    tis = np.concatenate([np.concatenate([s, [H.SEPARATOR]])
                          for s in seqs])[:-1].astype(np.uint8)
    other = [tis[a:a + 64].copy() for a in (5, 3100, 6500, 8800)]
    for i, r in enumerate(other):
        assert r.max() < 4
        r[10 + 11 * i] = (r[10 + 11 * i] + 1) % 4
    onemore = read.copy()
    onemore[50] = (onemore[50] + 2) % 4
    reads = [other[0], read, other[1], onemore, other[2], other[3]]
    each = [piece_hits(tis, len(tis), r, doedist, 1) for r in reads]
    assert each[1] == target, (each, target)
    return Case("hits%d_%s" % (target, kind), tis, reads, doedist, 1,
                uniform=True, words=1, hits=(each[1], sum(each)))


def last_read_case(m, packed):
    """the last read of the buffer with m % 8 in (1, 7): the band's 8-byte
    pattern load of its last row block reaches behind the read.  As bytes
    with reads of other lengths in front (nothing behind the last read), and
    as a batch of one length (which also runs packed)"""
    assert m % 8 in (1, 7)
    pool = border_reads("short", m, 2, True)
    if packed:
        reads = [pool[i] for i in (0, 4, 8, 13, 2)]
    else:
        reads = [border_reads("short", 96, 2, True)[3],
                 border_reads("short", 152, 2, True)[7], pool[0], pool[2]]
    return Case("last_m%d_%s" % (m, "uniform" if packed else "ragged"),
                text("short"), reads, True, 2, uniform=packed, words=words(m))


def too_long_reads():
    """a read of 513 symbols (VSA_APM_MAXWORDS * 64 + 1) and a batch that ends
    in it.  The engine declines both batches as a whole: VsaError with code
    NOT_COVERED, no partial list -- unlike the reference's own errors, which
    leave the reads in front answered."""
    tis = text("long")
    long = tis[:513].copy()
    assert long.max() < 4
    # (substitutions only: they answer under both distances)
    front = [border_reads("long", 512, 2, False)[1],
             border_reads("long", 128, 2, False)[5]]
    return tis, front, long


GROUPS = {
    "band_short": [("band", m) for m in [63, 64, 65] + BAND_LENGTHS +
                   [127, 128, 129]],
    "band_mid": [("band", m) for m in LENGTHS if 129 < m <= 321],
    "band_long": [("band", m) for m in LENGTHS if m > 321],
    "scan_short": [("scan", m) for m in LENGTHS if m <= 257],
    "scan_long": [("scan", m) for m in LENGTHS if m > 257],
    "hamming_short": [("hamming", m) for m in LENGTHS if m <= 257],
    "hamming_long": [("hamming", m) for m in LENGTHS if m > 257],
}


def group(name):
    return [uniform_case(kind, m) for kind, m in GROUPS[name]]


def mixed_cases():
    """W = 8 and W = 6 batches for the band (K = 2, also forced through the
    scan), the scan (K = 4) and Hamming distance (K = 2); 1 percent of 127 ..
    384 symbols = thresholds 1, 2 and 3 in one batch, whose band is that of
    K = 3"""
    out = []
    for longest in (512, 384):
        out += [mixed_case("band", longest, 2), mixed_case("scan", longest, 4),
                mixed_case("hamming", longest, 2)]
    out += [mixed_case("band", 384, 1, percent=1),
            mixed_case("hamming", 384, 1, percent=1)]
    ks = set(out[-2].thresholds())
    assert ks == {1, 2, 3}, ks
    return out


def plan_cases(kind="band"):
    """the same mixed reads planned in the three ways of apm_plan: one length
    (uniform), thresholds and piece lengths per read uploaded as vectors (up
    to TABLE_READS reads), per-length tables filled on the device (more)"""
    return [mixed_case(kind, 129, 2, copies=TABLE_READS),
            mixed_case(kind, 129, 2, copies=TABLE_READS + 1)]


_index, _expected = {}, {}


def host_index(tis):
    """the tables of a text from the CPU builder, made once"""
    key = tis.tobytes()
    if key not in _index:
        _index[key] = H.oracle_build_index(tis, 4)
    return _index[key]


def expected(case):
    """-> (the oracle's list, the model's set) of a case, computed once.  A
    batch repeated cyclically asks the model for its first round only."""
    import approx_model as A
    if case.name not in _expected:
        want = H.oracle_approx(host_index(case.text), case.queries(),
                               case.doedist, case.k, case.percent)
        period = len(case.reads)
        for i in range(1, len(case.reads)):
            if case.reads[i] is case.reads[0]:
                period = i
                break
        assert all(case.reads[i] is case.reads[i % period]
                   for i in range(len(case.reads)))
        one = A.matches(case.text, case.reads[:period], case.doedist, case.k,
                        case.percent)
        parts = []
        for base in range(0, len(case.reads), period):
            part = one[one["queryseq"] < len(case.reads) - base].copy()
            part["queryseq"] += base
            parts.append(part)
        _expected[case.name] = (want, A.as_set(np.concatenate(parts)))
    return _expected[case.name]


def check_exercised(case, want):
    """a case must meet what it was built for: matches flush to the first and
    to the last symbol of a sequence (the first sequence starts at text
    position 0, the last ends at n - 1), distances 0 and k"""
    assert len(want) > 0
    dist = set(int(d) for d in want["querystart"])
    assert 0 in dist and int(case.thresholds().max()) in dist, dist
    if case.border:
        seqs = sequences(case.text)
        first = set(a for a, L in seqs)
        last = set(a + L for a, L in seqs)
        starts = set(int(x) for x in want["dbstart"])
        ends = set(int(x) for x in want["dbstart"] + want["length"])
        assert first <= starts and last <= ends, (first - starts, last - ends)
