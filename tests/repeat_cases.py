"""Seeded texts for the repeat family (vmatch -l L IDX, -supermax, -tandem) at
the edges of its kernels (vstree_amd/csrc/selfmatch_search.inc), shared by the
CPU test (test_repeat_model_host.py), the GPU test (test_gpu_repeat_edges.py)
and the script that records the reference's lists
(scripts/make_golden_repeat_edges.py).  DNA alphabet throughout.

  nested  copies of U[:d], d = 253 .. 257 and 300, in different left and
          right contexts: rows of lcp exceptions with values below, equal to
          and above a node's depth, bytes of 253 and 254 next to them, search
          lengths on both sides of 255 (LcpCursor, lcp_select at lmin = 255)
  nested_tandem  V[:d] V[:d] V[:100], d = 254, 255, 256; two squares of 257
          symbols at the right end of their interval, an exception of 256
          behind it
  copies  300 identical sequences: one run of 300 suffixes whose left
          characters are all special (k_supermax_write, the special-class
          branches of k_rep_write); copies_small: 60 of them, for the model
  star    120 copies of a unit, continued by 0 .. 3 symbols of two fixed
          tails: children that are subtrees, and one attachment with every
          left-character class on both sides; star_cut: the same text as
          database and queries
  runs    runs of one symbol thousands long (key widths, k_tan_extent);
          runs_small for the model; runs_tail: runs of hundreds with room
          behind them
  tiny_*  texts of 1 .. 33 symbols (lcpsel_mask's 17 bytes, its guards)

case(name) -> Case: the text, the search lengths, the engines, the host
index (built by the CPU oracle) and the check of the case's own situation on
the host tables."""
import hashlib

import numpy as np

import helpers as H

SEP, WC = H.SEPARATOR, H.WILDCARD
FLANKS = (0, 1, 2, 3, WC, SEP)
ENGINES = ("repeats", "supermax", "tandem")
NESTED_DEPTHS = (253, 254, 255, 256, 257, 300)


def _rand(rng, k):
    return rng.integers(0, 4, k).astype(np.uint8)


def _join(parts):
    return np.concatenate([np.asarray(p, np.uint8) for p in parts])


def nested():
    rng = np.random.default_rng(25500)
    u = _rand(rng, 300)
    parts, k = [u[:256]], 0
    for d in NESTED_DEPTHS:
        for c in range(3):
            parts += [_rand(rng, 37), [FLANKS[k % 6]], u[:d],
                      [FLANKS[(k + 3 + k // 6) % 6]]]
            k += 1
    parts += [_rand(rng, 37), [1], u[:255]]
    return _join(parts), (200, 254, 255, 256, 257, 258, 300, 301)


def nested_tandem():
    rng = np.random.default_rng(25501)
    v = _rand(rng, 300)
    parts = []
    for i, d in enumerate((254, 255, 256)):
        if i:
            parts.append([SEP])
        parts += [_rand(rng, 20), v[:d], v[:d], v[:100]]
    # two squares X X of 257 symbols that are the last two suffixes of X's
    # interval (X[0] = 3 is the largest continuation), so that the witness is
    # the interval's right end; behind them, in the suffix array, X[:256] with
    # a larger next symbol: to the right of the interval's first position the
    # exceptions 257, >= 514, 256
    x = _rand(rng, 257)
    x[0], x[256] = 3, 0
    parts += [[SEP], _rand(rng, 20), x, x, [1], _rand(rng, 20), x, x, [2],
              _rand(rng, 20), x[:256], [2], _rand(rng, 600)]
    return _join(parts), (254, 255, 256, 257, 258)


def _copies(count):
    rng = np.random.default_rng(25502)
    w = _rand(rng, 20)
    parts = []
    for i in range(count):
        if i:
            parts.append([SEP])
        parts.append(w)
    return _join(parts), (5, 20)


def copies():
    return _copies(300)


def copies_small():
    return _copies(60)


def star():
    rng = np.random.default_rng(25503)
    unit = _rand(rng, 25)
    # copy c is followed by the first c mod 4 symbols of one of two fixed
    # tails that start differently: two large subtrees below the unit's node,
    # each with every left character, so that one of them is attached to a
    # father that holds the other
    tails = (np.array([1, 3, 0], np.uint8), np.array([2, 0, 3], np.uint8))
    parts = [unit, _rand(rng, 9)]          # the unit itself at position 0
    for c in range(120):
        parts += [[FLANKS[c % 6]], unit, tails[(c // 4) % 2][:c % 4],
                  [FLANKS[(c // 6 + c) % 6]], _rand(rng, 9)]
    return _join(parts), (10, 25, 27)


def star_cut():
    tis, lengths = star()
    return tis, lengths


def runs():
    return _join([np.zeros(3000), [1], np.zeros(2000), [WC],
                  np.full(1500, 3)]), (1, 300, 1999, 2000)


def runs_small():
    return _join([np.zeros(60), [1], np.zeros(40), [WC],
                  np.full(30, 3)]), (1, 6, 39, 40)


def runs_tail():
    """runs of hundreds in front of 1 400 random symbols: every interval of
    the runs, and every suffix next to one in the suffix array, has room for
    twice its depth in front of the end of the text"""
    rng = np.random.default_rng(25504)
    return _join([np.zeros(600), [1], np.zeros(400), [WC], np.full(300, 3),
                  [SEP], _rand(rng, 1400)]), (100, 255, 300, 599)


TINY = {
    "tiny_a": [0], "tiny_aa": [0, 0], "tiny_aaa": [0, 0, 0],
    "tiny_acac": [0, 1, 0, 1], "tiny_a_a": [0, SEP, 0],
    "tiny_naan": [WC, 0, 0, WC], "tiny_a15": [0] * 15, "tiny_a16": [0] * 16,
    "tiny_a17": [0] * 17, "tiny_a32": [0] * 32, "tiny_a33": [0] * 33,
    "tiny_ac8a": [0, 1] * 8 + [0],
}

BUILDERS = {"nested": nested, "nested_tandem": nested_tandem,
            "copies": copies, "copies_small": copies_small, "star": star,
            "star_cut": star_cut, "runs": runs, "runs_small": runs_small,
            "runs_tail": runs_tail}
for _name, _t in TINY.items():
    BUILDERS[_name] = (lambda t=_t: (np.array(t, np.uint8), (1, 2)))

# the definitional model (repeat_model.py) answers these at full size; copies
# and the runs are held against it through their smaller siblings
SIBLING = {"copies": "copies_small", "runs": "runs_small",
           "runs_tail": "runs_small"}
MODELLED = [c for c in BUILDERS if c not in SIBLING]
# the reference's lists are recorded for these (the siblings exist for the
# model alone)
RECORDED = [c for c in BUILDERS if c not in ("copies_small", "runs_small")]
NAMES = sorted(BUILDERS)


class Case:
    def __init__(self, name):
        self.name = name
        tis, lengths = BUILDERS[name]()
        self.tis = np.ascontiguousarray(tis, np.uint8)
        self.lengths = tuple(lengths)
        self.n = len(self.tis)
        self.ssp = np.flatnonzero(self.tis == SEP).astype(np.uint64)
        # star_cut: the sequences behind the middle separator are queries
        self.hasqueries = name == "star_cut"
        self.numofdbsequences = len(self.ssp) + 1
        self.qsep = 0
        if self.hasqueries:
            self.numofdbsequences = (len(self.ssp) + 1) // 2
            self.qsep = int(self.ssp[self.numofdbsequences - 1])
        self.engines = ("repeats",) if self.hasqueries else ENGINES
        self._host = None

    def md5(self):
        return hashlib.md5(self.tis.tobytes()).hexdigest()

    def records(self):
        """the sequences of the text as FASTA records"""
        bounds = np.concatenate(([-1], self.ssp.astype(np.int64), [self.n]))
        return [("%s_%d" % (self.name, i), self.tis[a + 1:b])
                for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:]))]

    def runs(self):
        """(engine, L) of every search of the case"""
        return [(e, L) for e in self.engines for L in self.lengths]

    @property
    def host(self):
        if self._host is None:
            idx = H.oracle_build_index(self.tis, 4, None, ssp=self.ssp,
                                       querysepposition=self.qsep,
                                       hasqueries=self.hasqueries)
            idx.numofdbsequences = self.numofdbsequences
            self._host = idx
        return self._host

    def oracle(self, engine, L):
        """the CPU oracle's list; OracleError where it raises one"""
        fn = {"repeats": H.oracle_repeats, "supermax": H.oracle_supermax,
              "tandem": H.oracle_tandems}[engine]
        return fn(self.host, L)

    def as_ref(self, m):
        conv = H.selfmatches_as_ref if self.hasqueries else H.repeats_as_ref
        return conv(self.host, m)

    def check_situation(self):
        check = SITUATIONS.get(self.name.split("_")[0] if
                               self.name.startswith("tiny") else self.name)
        if check is not None:
            check(self)


_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


_oracle = {}


def expected(name, engine, L):
    """the oracle's list of one search, computed once and never changed"""
    key = (name, engine, L)
    if key not in _oracle:
        m = case(name).oracle(engine, L)
        m.setflags(write=False)
        _oracle[key] = m
    return _oracle[key]


# ---- host tables --------------------------------------------------------------

def full_lcp(idx):
    """lcp values with the exceptions of llv filled in"""
    lcp = idx.lcp.astype(np.int64)
    if idx.nllv:
        llv = idx.llv.reshape(-1, 2).astype(np.int64)
        assert np.array_equal(llv[:, 0], np.flatnonzero(idx.lcp == 255))
        lcp[llv[:, 0]] = llv[:, 1]
    return lcp


def candidates(idx, engine, L):
    """the rule in the comment above lcpsel_mask on the host's lcp bytes:
    positions i < n whose byte lcp[i+1] is >= min(L, 255) and not 0; for
    -supermax additionally a rise lcp[i] < lcp[i+1], position 0 or a byte of
    255"""
    b = idx.lcp.astype(np.int64)
    here, nxt = b[:-1], b[1:]
    ok = (nxt >= min(L, 255)) & (nxt != 0)
    if engine == "supermax":
        ok &= (np.arange(idx.n) == 0) | (here < nxt) | (nxt == 255)
    return int(ok.sum())


def attachments(idx, L):
    """maximal repeats' units of work: for every p with lcp[p] = d >= L the
    father's part [l, p - 1] and the child [p, e] -> [(p, l, e, d)]"""
    lcp, out = full_lcp(idx), []
    for p in np.flatnonzero(lcp >= L):
        d, l, e = lcp[p], p - 1, p
        while lcp[l] >= d:
            l -= 1
        while e + 1 <= idx.n and lcp[e + 1] > d:
            e += 1
        out.append((int(p), int(l), int(e), int(d)))
    return out


def mixed_right_rows(idx, L):
    """how many lcp-intervals of depth d >= max(L, 255), named by their first
    position p, have to the right of p a row of exceptions that begins with
    a value >= d and holds a value < d further on: the right-hand walk of
    such an interval ends inside the row, at an exception it can only tell
    from the ones before it by its own entry of llv"""
    lcp, byte, count = full_lcp(idx), idx.lcp, 0
    exc = np.flatnonzero(byte == 255)
    if len(exc) == 0:
        return 0
    for row in np.split(exc, np.flatnonzero(np.diff(exc) != 1) + 1):
        v = lcp[row]
        # after[i]: the smallest value from i on.  Entry i is the first
        # position of its interval when the nearest value <= v[i] to its left
        # is smaller than v[i]; the byte in front of the row always is
        after = np.minimum.accumulate(v[::-1])[::-1]
        stack = []
        for i in range(len(v) - 1):
            while stack and v[stack[-1]] > v[i]:
                stack.pop()
            first = not stack or v[stack[-1]] < v[i]
            stack.append(i)
            if first and v[i] >= L and v[i + 1] >= v[i] and after[i + 1] < v[i]:
                count += 1
    return count


def _classes(bwt):
    return set(int(min(c, 4)) for c in bwt)


# ---- the situations the cases exist for ---------------------------------------

def _nested_situation(c):
    idx, lcp = c.host, full_lcp(c.host)
    byte = idx.lcp
    exc = np.flatnonzero(byte == 255)
    assert len(exc) >= 40, len(exc)
    inner = [q for q in exc if byte[q - 1] == 255 and q + 1 <= c.n
             and byte[q + 1] == 255]
    assert inner, "no exception with exceptions on both sides"
    seen = {-1: set(), 1: set()}
    for q in inner:
        for side in (-1, 1):
            w = lcp[q + side]
            seen[side].add("below" if w < lcp[q] else
                           "equal" if w == lcp[q] else "above")
    assert seen[-1] == seen[1] == {"below", "equal", "above"}, seen
    depths = set(int(v) for v in lcp[exc])
    assert depths >= {255, 256, 257, 300}, depths
    for small in (253, 254):
        q = np.flatnonzero(byte == small)
        assert ((byte[q - 1] == 255) | (byte[np.minimum(q + 1, c.n)]
                                        == 255)).any(), small
    # a repeat of 255 and more symbols that ends with the text, another one
    # that starts it
    suf = idx.suf.astype(np.int64)
    ends = [q for q in exc if suf[q] + lcp[q] == c.n
            or suf[q - 1] + lcp[q] == c.n]
    assert ends and any(suf[q] == 0 or suf[q - 1] == 0 for q in exc)
    assert mixed_right_rows(idx, 200) >= 3


def _nested_tandem_situation(c):
    for L, least in ((254, 5), (255, 4), (256, 3), (257, 2), (258, 0)):
        m = expected(c.name, "tandem", L)
        assert len(m) >= least and (least > 0 or len(m) == 0), (L, len(m))
        assert all(int(x) >= L for x in m["length"])
    assert set(int(x) for x in expected(c.name, "tandem", 254)["length"]) \
        >= {254, 255, 256, 257}
    assert mixed_right_rows(c.host, 257) >= 1


def _copies_situation(c, count=300):
    idx, lcp = c.host, full_lcp(c.host)
    s = np.flatnonzero((lcp[:-1] < 20) & (lcp[1:] == 20))
    assert len(s) == 1
    s = int(s[0])
    assert (lcp[s + 1:s + count] == 20).all() and lcp[s + count] < 20
    assert (idx.bwt[s:s + count] >= 253).all()
    pairs = count * (count - 1) // 2
    for engine in ("repeats", "supermax"):
        for L in c.lengths:
            assert len(expected(c.name, engine, L)) == pairs


def _star_situation(c):
    idx = c.host
    every = {0, 1, 2, 3, 4}
    full = [a for a in attachments(idx, 10)
            if _classes(idx.bwt[a[1]:a[0]]) == every
            and _classes(idx.bwt[a[0]:a[2] + 1]) == every]
    assert full, "no attachment with every class on both sides"
    p, l, e, d = max(full, key=lambda a: a[2] - a[1])
    assert e - l + 1 >= 100 and p - l >= 10 and e - p + 1 >= 10
    # children that are subtrees: deeper nodes below the unit's node
    lcp = full_lcp(idx)
    assert (lcp[l + 1:e + 1] > d).any()
    whole = len(expected("star", "repeats", 10))
    assert whole >= 5000
    if c.hasqueries:
        # the pairs of a database and a query position: some kept, some not
        assert 1000 <= len(expected(c.name, "repeats", 10)) <= whole - 1000
    else:
        assert len(expected(c.name, "supermax", 10)) >= 20


def _runs_situation(c, deepest=2999, least=2000, rows=1000):
    lcp = full_lcp(c.host)
    assert lcp.max() >= deepest
    assert mixed_right_rows(c.host, c.lengths[0]) >= rows
    assert len(expected(c.name, "tandem", c.lengths[0])) >= least
    assert len(expected(c.name, "repeats", c.lengths[0])) >= 5 * least


def _tiny_situation(c):
    assert 1 <= c.n <= 33


SITUATIONS = {
    "nested": _nested_situation, "nested_tandem": _nested_tandem_situation,
    "copies": _copies_situation,
    "copies_small": lambda c: _copies_situation(c, 60),
    "star": _star_situation, "star_cut": _star_situation,
    "runs": _runs_situation,
    "runs_small": lambda c: _runs_situation(c, 59, 40, 0),
    "runs_tail": lambda c: _runs_situation(c, 599, 300, 100),
    "tiny": _tiny_situation,
}
