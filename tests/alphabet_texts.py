"""Seeded texts and queries over alphabets of 2 .. 253 symbols for
tests/test_gpu_alphabets.py, and what the CPU oracle reports on them (computed
once per alphabet, shared by the tests, never changed).  Test infrastructure;
no GPU involved here."""
import numpy as np

import helpers as H

SWEEP = (2, 3, 5, 7, 8, 9, 16, 17, 20, 31, 32, 33, 64, 65, 128, 129, 200, 253)
REP_MAXC = 32          # maximal repeats: alphabets beyond are declined
SELFMUM_MAXC = 128     # self-MUM scan: alphabets beyond are declined


def substitute(rng, s, k, nc):
    s = s.copy()
    for _ in range(k):
        p = int(rng.integers(0, len(s)))
        s[p] = (int(s[p]) + 1 + int(rng.integers(0, max(1, nc - 1)))) % nc \
            if s[p] < nc else int(rng.integers(0, nc))
    return s


def sweep_sequences(nc):
    """three sequences of 4000 uniform symbols; a 120-symbol unit planted six
    times per sequence with 0-3 substitutions each; a period-3 tandem of 40
    symbols from the symbols nc-1, 0, nc-2; wildcards at 0.3 %; the unit's
    first 40 symbols at text position 0.  The 18 copies are nine variants of
    the unit, each planted twice behind two different symbols: every variant
    is a repeat of 120 symbols with exactly two occurrences that no longer
    repeat contains, so that supermaximal repeats of 40 and more symbols
    exist at every alphabet size."""
    rng = np.random.default_rng(1000 + nc)
    unit = rng.integers(0, nc, 120).astype(np.uint8)
    variants = [unit] + [substitute(rng, unit, 1 + v % 3, nc)
                         for v in range(8)]
    order = rng.permutation(18)
    seqs = [rng.integers(0, nc, 4000).astype(np.uint8) for s in range(3)]
    for slot, k in enumerate(order):
        t, r = seqs[slot // 6], slot % 6
        p = 100 + 640 * r + int(rng.integers(0, 500))
        t[p:p + 120] = variants[k // 2]
        t[p - 1] = k % 2
    for t in seqs:
        hit = np.flatnonzero(rng.random(4000) < 0.003)
        t[hit] = H.WILDCARD
    period = np.array([nc - 1, 0, max(nc - 2, 0)], np.uint8)
    seqs[1][3900:3940] = np.resize(period, 40)
    seqs[0][:40] = unit[:40]
    return seqs


def join(seqs):
    parts = []
    for i, s in enumerate(seqs):
        if i:
            parts.append(np.array([H.SEPARATOR], np.uint8))
        parts.append(np.asarray(s, np.uint8))
    return np.concatenate(parts)


def sweep_queries(nc, seqs, minlength):
    """300 substrings of minlength .. 90 symbols, half with one substitution"""
    rng = np.random.default_rng(2000 + nc)
    out = []
    for i in range(300):
        s = seqs[int(rng.integers(0, 3))]
        m = int(rng.integers(minlength, 91))
        p = int(rng.integers(0, len(s) - m))
        q = s[p:p + m]
        out.append(substitute(rng, q, 1, nc) if i % 2 else q.copy())
    return H.Queries.from_list(out)


def query_lengths(nc, pl):
    """search lengths of the query modes: max(pl, 3) and 8; on the smallest
    alphabets 8 and 12 (3 gives a million matches there); never below pl"""
    base = (8, 12) if nc <= 5 else (max(pl, 3), 8)
    return sorted(set(max(pl, L) for L in base))


def forced_prefixlength(plrec):
    """the second prefix length of the alphabets from 20 symbols on: 1, and
    where the recommendation is 1 already (31 symbols and more on these
    texts) 2, so that the q-gram code of more than one symbol runs"""
    return 1 if plrec != 1 else 2


MODES = (("mem_sp0", dict(speedup=0)), ("mem_sp2", dict(speedup=2)),
         ("mumcand", dict(mum=True, cand=True, speedup=2)),
         ("mum", dict(mum=True, speedup=2)))

_sweep = {}


def sweep_case(nc):
    """-> dict: text, queries, per prefix length the oracle's index and its
    lists of every query mode, the lists of the repeat family and of the
    self-MUM scan"""
    if nc in _sweep:
        return _sweep[nc]
    seqs = sweep_sequences(nc)
    tis = join(seqs)
    plrec = H.recommended_prefixlength(nc, len(tis))
    pls = [plrec] + ([forced_prefixlength(plrec)] if nc >= 20 else [])
    # no read below a prefix length: that is -complete's hard error
    queries = sweep_queries(nc, seqs, max(pls))
    c = dict(nc=nc, tis=tis, queries=queries, plrec=plrec, index={},
             query={}, sizes={})
    for pl in pls:
        idx = H.oracle_build_index(tis, nc, pl)
        c["index"][pl] = idx
        want = {"complete": H.oracle_complete(idx, queries)}
        for L in query_lengths(nc, pl):
            for name, kw in MODES:
                want["%s%d" % (name, L)] = H.oracle_querymatches(
                    idx, queries, L, **kw)
        c["query"][pl] = want
        c["sizes"]["pl%d" % pl] = {k: len(v) for k, v in want.items()}
    idx = c["index"][plrec]
    c["supermax"] = {L: H.oracle_supermax(idx, L) for L in (3, 8, 40)}
    c["tandem"] = {L: H.oracle_tandems(idx, L) for L in (1, 3)}
    c["repeats"] = ({L: H.oracle_repeats(idx, L) for L in (8, 40)}
                    if nc <= REP_MAXC else {})
    # database | separator | the first 2000 symbols of the second sequence:
    # an index that holds its queries
    both = np.concatenate([tis, [H.SEPARATOR], seqs[1][:2000]]).astype(
        np.uint8)
    c["selftis"], c["selfsep"] = both, len(tis)
    if nc <= SELFMUM_MAXC:
        sidx = H.oracle_build_index(both, nc, plrec,
                                    querysepposition=len(tis),
                                    hasqueries=True)
        c["selfindex"] = sidx
        c["selfmum"] = H.oracle_selfmum(sidx, 8)
    for k in ("supermax", "tandem", "repeats"):
        c["sizes"][k] = {L: len(v) for L, v in c[k].items()}
    c["sizes"]["selfmum8"] = len(c["selfmum"]) if "selfmum" in c else None
    _sweep[nc] = c
    return c


# What the CPU oracle reports on the sweep texts, per alphabet size, at the
# recommended prefix length (the forced one gives the same lists):
#   (pl, -complete, MEM at the two L, MUM candidates, MUM, supermax at L = 3 /
#    8 / 40, tandem at L = 1 / 3, repeats at L = 8 / 40, self-MUM at L = 8);
# None: declined by the engine at that size.  tests/test_oracle_alphabets.py
# asserts the table, so that a reader sees that no comparison is empty.
SIZES = {
    2: (9, 361, (148998, 17927), (799, 792), (393, 391), (1674, 1674, 23), (5932, 1414), (137662, 168), 8),
    3: (6, 324, (16517, 1944), (693, 316), (378, 224), (2121, 1929, 18), (4075, 532), (7314, 178), 8),
    5: (4, 435, (2594, 1807), (338, 288), (235, 213), (2681, 117, 16), (2398, 70), (751, 150), 7),
    7: (3, 406, (402359, 1898), (581, 344), (321, 232), (3005, 33, 17), (1727, 45), (608, 185), 6),
    8: (3, 388, (273084, 2006), (537, 320), (287, 219), (3636, 26, 14), (1377, 24), (612, 132), 2),
    9: (3, 253, (189375, 2265), (590, 337), (327, 230), (3577, 19, 14), (1273, 25), (610, 160), 5),
    16: (2, 433, (35027, 2311), (518, 320), (289, 223), (5469, 22, 17), (703, 10), (606, 179), 11),
    17: (2, 386, (33905, 2550), (542, 331), (306, 245), (5359, 21, 12), (658, 8), (608, 149), 14),
    20: (2, 363, (21457, 2190), (546, 346), (282, 236), (4361, 21, 14), (605, 9), (559, 163), 8),
    31: (1, 288, (8126, 1883), (486, 349), (284, 230), (1479, 19, 11), (486, 6), (573, 154), 7),
    32: (1, 279, (7911, 2126), (479, 334), (272, 232), (1292, 20, 11), (368, 6), (587, 171), 4),
    33: (1, 279, (7972, 1921), (475, 346), (267, 227), (1245, 16, 11), (359, 6), None, 6),
    64: (1, 230, (3666, 2140), (380, 324), (259, 236), (171, 13, 10), (208, 6), None, 8),
    65: (1, 211, (3704, 2365), (394, 334), (263, 235), (186, 15, 12), (154, 6), None, 7),
    128: (1, 226, (3055, 1987), (387, 324), (249, 225), (41, 13, 11), (103, 6), None, 6),
    129: (1, 219, (2904, 2067), (388, 329), (250, 228), (36, 15, 12), (108, 6), None, None),
    200: (1, 247, (2830, 2151), (384, 327), (245, 224), (23, 14, 12), (53, 6), None, None),
    253: (1, 280, (3484, 2429), (387, 333), (236, 223), (14, 13, 11), (47, 6), None, None),
}


def list_sizes(c):
    """a sweep_case in the layout of SIZES"""
    q, Ls = c["query"][c["plrec"]], query_lengths(c["nc"], c["plrec"])
    return (c["plrec"], len(q["complete"]),
            tuple(len(q["mem_sp0%d" % L]) for L in Ls),
            tuple(len(q["mumcand%d" % L]) for L in Ls),
            tuple(len(q["mum%d" % L]) for L in Ls),
            tuple(len(c["supermax"][L]) for L in (3, 8, 40)),
            tuple(len(c["tandem"][L]) for L in (1, 3)),
            (tuple(len(c["repeats"][L]) for L in (8, 40))
             if c["repeats"] else None),
            len(c["selfmum"]) if "selfmum" in c else None)


def many_classes_text(nc):
    """Maximal repeats with many left-character classes at one node: a
    30-symbol unit U at text position 0; for every symbol c the block
    [c] + U[:30 - 5 (c % 4)] + [(7 c + rep) % nc] + 6 random symbols, written
    twice for c % 3 == 0 (two father elements of one class, whose pairs are
    skipped); then [WILDCARD] + U + [1], [SEPARATOR] + U + [2, WILDCARD] + U"""
    rng = np.random.default_rng(3000 + nc)
    U = rng.integers(0, nc, 30).astype(np.uint8)
    parts = [U]
    for c in range(nc):
        for rep in range(2 if c % 3 == 0 else 1):
            parts += [[c], U[:30 - 5 * (c % 4)], [(7 * c + rep) % nc],
                      rng.integers(0, nc, 6)]
    parts += [[H.WILDCARD], U, [1], [H.SEPARATOR], U, [2, H.WILDCARD], U]
    return np.concatenate([np.asarray(p, np.uint8) for p in parts])


def high_left_symbols_text():
    """Supermaximal repeats whose left symbols differ only above bit 5:
    200 symbols, 3000 uniform ones; a 25-symbol unit V planted three times
    behind 5, 69 and 133 (equal modulo 64) and in front of three different
    symbols; a 25-symbol unit W planted three times behind 70, 70 and 6"""
    nc = 200
    rng = np.random.default_rng(4000)
    t = rng.integers(0, nc, 3000).astype(np.uint8)
    V = rng.integers(0, nc, 25).astype(np.uint8)
    W = rng.integers(0, nc, 25).astype(np.uint8)
    for p, left, right in ((200, 5, 11), (700, 69, 12), (1200, 133, 13)):
        t[p - 1], t[p + 25] = left, right
        t[p:p + 25] = V
    for p, left, right in ((1700, 70, 21), (2200, 70, 22), (2700, 6, 23)):
        t[p - 1], t[p + 25] = left, right
        t[p:p + 25] = W
    return nc, t
