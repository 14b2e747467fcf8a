"""A plain model of approximate complete matches (vmatch -complete -e K |
-h K) for reads WITHOUT special symbols: no pieces, no regions, no bit
vectors -- every start position of the text is asked the same question.

Edit distance, threshold k, read P of m symbols, text T of n symbols:
  start position p is reported iff T[p] is no separator and the smallest
  unit edit distance between P and one of the prefixes T[p .. p+j),
  j = 1 .. min(m + k, n - p), none of them reaching into a separator, is
  <= k.  The record is (length = the LARGEST j that attains the smallest
  distance, dbstart = p, queryseq, querystart = that distance).
Hamming distance, threshold k:
  p is reported iff p + m <= n, no separator lies in T[p .. p+m) and the
  number of mismatches is <= k; the record is (m, p, queryseq, mismatches).
A wildcard of the text equals nothing.

The model gives a SET per read; the order of a list is the oracle's
business.  `edit_at` is the definition for one start position, cell by cell;
`matches` asks all start positions at once (numpy over (read, start) pairs)
and is held against `edit_at` by tests/test_approx_model_host.py.

Two facts keep the vectorised form small, both consequences of the
definition and of unit costs:
  * an alignment with <= k errors never leaves the diagonals |row - column|
    <= k, so only those 2k + 1 cells of a row are kept, values above k held
    at k + 1;
  * a start position whose row has no cell <= k cannot be reported any more
    and is dropped.
"""
import numpy as np

SEPARATOR = 255
WILDCARD = 254
MATCH_DTYPE = np.dtype([("length", "<u8"), ("dbstart", "<u8"),
                        ("queryseq", "<u8"), ("querystart", "<u8")])


def symbols_before_separator(text):
    """free[p] = symbols from p on in front of the next separator or the end
    of the text (0 where T[p] is a separator)"""
    n = len(text)
    stops = np.concatenate([np.flatnonzero(text == SEPARATOR), [n]])
    p = np.arange(n)
    return stops[np.searchsorted(stops, p)] - p


def edit_at(text, read, p, k):
    """the definition at one start position, cell by cell -> (length,
    distance) or None"""
    n, m = len(text), len(read)
    if text[p] == SEPARATOR:
        return None
    col = list(range(m + 1))            # distances to the empty prefix
    best = None
    for j in range(1, min(m + k, n - p) + 1):
        c = int(text[p + j - 1])
        if c == SEPARATOR:
            break
        new = [j] + [0] * m
        for i in range(1, m + 1):
            new[i] = min(col[i - 1] + (0 if int(read[i - 1]) == c and
                                       c != WILDCARD else 1),
                         col[i] + 1, new[i - 1] + 1)
        col = new
        if best is None or col[m] <= best[1]:
            best = (j, col[m])
    return best if best is not None and best[1] <= k else None


def hamming_at(text, read, p, k):
    n, m = len(text), len(read)
    if p + m > n or (text[p:p + m] == SEPARATOR).any():
        return None
    mm = int((text[p:p + m] != read).sum())
    return (m, mm) if mm <= k else None


def _edit_pairs(tp, free, reads, r, p, k):
    """reads: (R, m) symbols; (r[i], p[i]): read r[i] at start position p[i]
    -> (r, p, length, distance) of the pairs that are reported"""
    m, w, inf = reads.shape[1], 2 * k + 1, k + 1
    e = np.arange(w)
    lim = np.minimum(free[p], m + k)     # columns 1 .. lim are text of p
    keep = lim > 0
    r, p, lim = r[keep], p[keep], lim[keep]
    # row 0: D[0][j] = j; cell e of row i is column j = i + e - k
    band = np.where((e - k >= 0)[None, :] & (e - k <= lim[:, None]),
                    (e - k)[None, :], inf).astype(np.int16)
    # win[p + i] = the text symbols of columns i - k .. i + k of start p
    # (columns <= 0 read what lies in front of p and are not used)
    win = np.lib.stride_tricks.sliding_window_view(
        np.concatenate([np.full(k + 1, SEPARATOR, np.uint8), tp]), w)
    e = e.astype(np.int16)
    for i in range(1, m + 1):
        j = i + e - k
        v = band + (win[p + i] != reads[r, i - 1][:, None])    # diagonal
        v[:, :-1] = np.minimum(v[:, :-1], band[:, 1:] + 1)     # from above
        v[:, j < 0] = inf
        v[:, j == 0] = min(i, inf)
        v = np.minimum.accumulate(v - e, axis=1) + e           # from the left
        band = np.minimum(v, inf)
        band[j[None, :] > lim[:, None]] = inf
        alive = (band <= k).any(axis=1)
        if not alive.all():
            r, p, lim, band = r[alive], p[alive], lim[alive], band[alive]
    dist = band.min(axis=1)
    last = w - 1 - np.argmax(band[:, ::-1] == dist[:, None], axis=1)
    ok = dist <= k
    return r[ok], p[ok], (m + last - k)[ok], dist[ok]


def _hamming_pairs(tp, free, reads, r, p, k):
    m = reads.shape[1]
    keep = free[p] >= m
    r, p = r[keep], p[keep]
    mm = np.zeros(len(p), np.int64)
    for i in range(m):
        mm += tp[p + i] != reads[r, i]
        alive = mm <= k
        if not alive.all():
            r, p, mm = r[alive], p[alive], mm[alive]
    return r, p, np.full(len(p), m), mm


def matches(text, reads, doedist, distvalue, percent=0, starts=None):
    """reads: list of symbol arrays.  percent 0: threshold distvalue; 1:
    distvalue percent of the read's length; 2: best of -- the read's smallest
    distance within distvalue percent.  Threshold 0 is the exact search.
    starts: None = every position of the text, or one array of start
    positions per read (the model restricted to those).
    -> MATCH_DTYPE records sorted by (queryseq, dbstart)"""
    text = np.asarray(text, np.uint8)
    n = len(text)
    free = symbols_before_separator(text)
    maxm = max(len(q) for q in reads)
    tp = np.concatenate([text, np.full(2 * maxm + 2, SEPARATOR, np.uint8)])
    out = []
    for m in sorted(set(len(q) for q in reads)):
        which = np.array([i for i, q in enumerate(reads) if len(q) == m])
        block = np.array([reads[i] for i in which], np.uint8)
        assert (block < WILDCARD).all(), "the model is for reads without " \
            "special symbols"
        k = m * distvalue // 100 if percent else distvalue
        assert k < m
        if starts is None:
            r = np.repeat(np.arange(len(which)), n)
            p = np.tile(np.arange(n), len(which))
        else:
            r = np.concatenate([np.full(len(starts[i]), x, np.int64)
                                for x, i in enumerate(which)])
            p = np.concatenate([np.asarray(starts[i], np.int64)
                                for i in which])
        fn = _edit_pairs if (doedist and k > 0) else _hamming_pairs
        r, p, length, dist = fn(tp, free, block, r, p, k)
        if percent == 2 and len(r):
            best = np.full(len(which), k + 1)
            np.minimum.at(best, r, dist)
            keep = dist <= best[r]
            r, p, length, dist = r[keep], p[keep], length[keep], dist[keep]
        rec = np.zeros(len(r), MATCH_DTYPE)
        rec["length"], rec["dbstart"] = length, p
        rec["queryseq"], rec["querystart"] = which[r], dist
        out.append(rec)
    return as_set(np.concatenate(out))


def as_set(records):
    """a list as the set the model speaks of: sorted by (queryseq, dbstart),
    which is a key -- a read reports a start position once"""
    records = np.asarray(records)
    order = np.lexsort((records["dbstart"], records["queryseq"]))
    return records[order]
