"""The recorded runs of vmatch -l L -hxdrop X | -exdrop X
(tests/golden/extend_xdrop_manifest.json, extend_xdrop_expected.npz, written
by scripts/make_golden_extend_xdrop.py) on the inputs of extend_cases.RUNS,
and the seed lists made by hand for the border cases of the X-drop
extension.  Shared by the generator and the extend_xdrop test modules."""
import json
import os

import numpy as np

import extend_cases as EC
import extend_xdrop_model as XM
import helpers as H


def R(key, case, L, X, hamming, q=True, S=0, strands="d", alphabet=False,
      error=False):
    return dict(key=key, case=case, L=L, X=X, hamming=hamming, q=q, S=S,
                strands=strands, alphabet=alphabet, error=error)


# S = 0: no -seedlength, the seeds have 30 symbols
RUNS = [
    R("c5_q_l40_hx5", "c5", 40, 5, True),
    R("c5_q_l40_ex5", "c5", 40, 5, False),
    R("c5_q_l40_hx1_s20", "c5", 40, 1, True, S=20),
    R("c5_q_l40_ex2_s20", "c5", 40, 2, False, S=20),
    # FLAGXDROP: X is 1 .. 255
    R("c5_q_l40_hx256", "c5", 40, 256, True, error=True),
    R("at1mb_l60_hx20", "at1mb", 60, 20, True, q=False),
    R("at1mb_l60_ex20", "at1mb", 60, 20, False, q=False),
    R("at1mb_l100_ex255_s40", "at1mb", 100, 255, False, q=False, S=40),
    R("grumbach_q_l30_hx2_dp", "grumbach", 30, 2, True, strands="dp"),
    R("grumbach_q_l30_ex5_dp", "grumbach", 30, 5, False, strands="dp"),
    # (an index built with -db .. -q ..: database against query positions)
    R("grumbach_all_l30_hx5", "grumbach_all", 30, 5, True, q=False),
    R("grumbach_all_l30_ex20", "grumbach_all", 30, 20, False, q=False),
    R("micro_q_l8_hx1_s6", "micro", 8, 1, True, S=6),
    R("micro_q_l8_ex2_s6", "micro", 8, 2, False, S=6),
    R("wildcards_q_l8_hx2_s6", "wildcards", 8, 2, True, S=6),
    R("wildcards_q_l8_ex5_s6", "wildcards", 8, 5, False, S=6),
    R("wildcards_l6_hx1_s5", "wildcards", 6, 1, True, q=False, S=5),
    R("wildcards_l6_ex2_s5", "wildcards", 6, 2, False, q=False, S=5),
    R("prot_l12_hx5_s8", "prot", 12, 5, True, q=False, S=8, alphabet=True),
    R("prot_l12_ex5_s8", "prot", 12, 5, False, q=False, S=8, alphabet=True),
    R("prot_q_l12_hx2_s8", "prot", 12, 2, True, S=8, alphabet=True),
    R("prot_q_l12_ex20_s8", "prot", 12, 20, False, S=8, alphabet=True),
    # matches of thousands of symbols
    R("ychr3_l200_hx20", "largepat", 200, 20, True, q=False),
    R("ychr3_l200_ex20", "largepat", 200, 20, False, q=False),
]

load, passes, md5 = EC.load, EC.passes, EC.md5


def run_of(key):
    return next(r for r in RUNS if r["key"] == key)


def vmatch_args(r):
    a = {"d": [], "p": ["-p"], "dp": ["-d", "-p"]}[r["strands"]]
    a += ["-l", str(r["L"]), "-hxdrop" if r["hamming"] else "-exdrop",
          str(r["X"])]
    if r["S"]:
        a += ["-seedlength", str(r["S"])]
    return a


def oracle_seeds(r, queries):
    """the seed list of a pass from the CPU oracle, in reference order"""
    idx, _ = load(r)
    S = XM.seedlength_rule(r["S"])
    if queries is None:
        return H.oracle_repeats(idx, S)
    return H.oracle_querymatches(idx, queries, S, speedup=2)


def parse_rows(lines):
    """the default columns -> rows (length1, seq1, rel1, length2, seq2, rel2,
    distance as printed, palindromic)"""
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
    length2 = XM.lengths2(rec).astype(np.int64)
    out[:, 0] = XM.lengths1(rec)
    out[:, 1], out[:, 2] = idx.seq_rel(rec["dbstart"])
    out[:, 3] = length2
    out[:, 6] = XM.distances(rec).astype(np.int64) * (-1 if r["hamming"]
                                                      else 1)
    out[:, 7] = palindromic
    if r["q"]:
        out[:, 4] = rec["queryseq"]
        rel = XM.starts(rec).astype(np.int64)
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


def sink_kind(V, query, hamming):
    return {(True, True): V.SINK_QUERY_HXDROP,
            (False, True): V.SINK_SELF_HXDROP,
            (True, False): V.SINK_QUERY_EXDROP,
            (False, False): V.SINK_SELF_EXDROP}[bool(query), bool(hamming)]


def sink_kwargs(V, r, palindromic):
    kw = EC.sink_kwargs(V, dict(r, K=0), palindromic)
    kw["kind"] = sink_kind(V, r["q"], r["hamming"])
    return kw


_manifest = None
_arrays = None


def manifest():
    global _manifest
    if _manifest is None:
        with open(os.path.join(H.GOLDEN, "extend_xdrop_manifest.json")) as f:
            _manifest = json.load(f)
    return _manifest


def expected_rows(key):
    global _arrays
    if _arrays is None:
        _arrays = np.load(os.path.join(H.GOLDEN, "extend_xdrop_expected.npz"))
    return _arrays[key].astype(np.int64).reshape(-1, 8)


def golden_keys(error=False):
    return [r["key"] for r in RUNS if r["error"] == error]


# --------------------------------------------------------------------------
# seed lists made by hand: the border cases of the extension
# --------------------------------------------------------------------------

import extend_edist_cases as DC  # noqa: E402

SEP, WILD = H.SEPARATOR, H.WILDCARD


class Scenario(DC.Scenario):
    """DC.Scenario with params [(L, X, S, modes)]: modes "h", "e" or "he",
    the extensions the parameter set is run with"""

    def model(self, L, X, S, hamming, **variant):
        return XM.extend(self.records(), self.text, L, X, hamming, S,
                         self.triple(), **variant)


def adopt(sc, name, params):
    """a scenario of the edit-distance cases with parameters of ours"""
    sc.__class__ = Scenario
    sc.name, sc.params = name, params
    return sc


def _drops():
    """-hxdrop: a drop that lands on best - X (the side goes on) and one
    below it (it stops); two equal maxima (the first stays); S - 1 and S
    matches in a row left of the seed (kept / rejected); the same on the
    right, where no rule applies"""
    sc = Scenario("drops", 1500, 41)
    for X in (1, 2, 5):
        on = [(d, "s") for d in range(X)] + [(X + 6, "s")]
        off = [(d, "s") for d in range(X + 1)] + [(X + 7, "s")]
        for side in (on, off):
            sc.planted(100, 40, 12, 40, [], side, beside=False)
            sc.planted(100, 40, 12, 40, side, [], beside=False)
            # ... behind a first stretch of matches
            far = [(d + 4, w) for d, w in side]
            sc.planted(300, 40, 12, 40, far, far, beside=False)
    # M M x x M x x x x x x: 4 at two symbols and again at five
    twice = [(d, "s") for d in (2, 3, 5, 6, 7, 8, 9, 10, 11)]
    sc.planted(500, 40, 12, 40, twice, twice, beside=False)
    sc.planted(500, 40, 12, 40, [(2, "s"), (4, "s"), (6, "s")],
               [(1, "s"), (3, "s"), (5, "s"), (6, "s")], beside=False)
    # runs of 9, 10 and 11 matches between two mismatches (S = 10)
    for run in (9, 10, 11):
        sc.planted(700, 60, 12, 60, [(run + 1, "s")], [(run + 1, "s")])
        sc.planted(700, 60, 12, 60, [(3, "s"), (4 + run, "s")], [])
    # ... and directly beside a seed that is not maximal
    for run in (9, 10):
        sc.planted(900, 60, 12, 60, [(run, "s")], [(run, "s")], beside=False)
    sc.params = [(14, 1, 10, "he"), (14, 2, 10, "he"), (14, 5, 10, "he"),
                 (14, 3, 10, "e"), (20, 5, 0, "he"), (14, 255, 10, "he")]
    return sc


def _hspecials():
    """a wildcard facing the same wildcard, a separator directly beside the
    seed and a few symbols away, in the text, in the read and in both"""
    sc = Scenario("hspecials", 2500, 42)
    t = sc.text
    w = 60
    for d in (0, 1, 3, 7, 8, 9):
        t[w + 30 + 10 + d] = WILD
        sc.planted(w, 30, 10, 30, [(2, "s")], [(d, "W")], beside=False)
        sc.planted(w, 30, 10, 30, [(2, "s")], [(d + 1, "W")], beside=False)
        t[w + 30 - 1 - d] = WILD
        sc.planted(w, 30, 10, 30, [(d, "W")], [(12, "s")], beside=False)
        w += 100
    for d in (0, 1, 3, 7, 8, 9):
        t[w + 30 + 10 + d] = SEP
        sc.planted(w, 30, 10, 30, [(d, "S")], [], beside=False)
        sc.planted(w, 30, 10, 30, [], [(d + 2, "S")], beside=False)
        sc.planted(w, 30, 10, 30, [(d, "S")], [(d, "S")], beside=False)
        sc.planted(w, 30, 10, 30, [(1, "d"), (d + 2, "S")],
                   [(1, "i"), (max(d, 1) - 1, "S")], beside=False)
        w += 100
    assert w < 2400
    sc.params = [(10, 2, 8, "he"), (12, 5, 8, "he"), (10, 1, 8, "he"),
                 (10, 20, 8, "he")]
    return sc


def _slides(budget, step):
    """-hxdrop right sides and -exdrop slides of budget - 1 .. budget + 1 and
    step - 1 .. step + 1 matches, every start address modulo 8"""
    ctx = step + 60
    sc = Scenario("slides", 2 * ctx + 400, 43)
    for T in (7, 8, 9, budget - 1, budget, budget + 1, budget + 8, step - 1,
              step, step + 1):
        stop = [(T, "s"), (T + 1, "s"), (T + 2, "s")]
        sc.planted(50 + ctx, 10, 12, ctx, [(0, "s")], stop, beside=False)
        # (the left side rejects a seed behind S matches: S above them all)
        sc.planted(50, ctx, 12, 10, stop, [(0, "s")], beside=False)
        sc.planted(50 + ctx, 10, 12, ctx, [], [(1, "d")] +
                   [(d + 3, w) for d, w in stop])
    base = 2 * ctx + 100
    for i in range(8):
        q = sc.text[base + i:base + i + 63].copy()
        for o in (5, 6, 44, 45):
            q[o] = sc.other(q[o])
        sc.reads.append(q)
        for o in range(20, 28):
            sc.seed(len(sc.reads) - 1, o, 4, base + i + o)
    sc.params = [(14, 1, 100000, "he"), (14, 2, 100000, "he"),
                 (14, 2, 40, "h")]
    return sc


def _manygenerations():
    """a difference every 9 or 10 symbols over 1500 symbols: more generations
    than the ring of T values holds"""
    sc = Scenario("manygenerations", 3600, 44)
    for w, step in ((100, 9), (1800, 10)):
        edits = [(int(x), "sid"[i % 3]) for i, x in
                 enumerate(range(3, 1500, step))]
        sc.planted(w, 1550, 12, 100, edits, [(5, "s")])
        sc.planted(w, 100, 12, 1550, [(5, "s")], edits)
    sc.params = [(40, 20, 100000, "e"), (40, 255, 100000, "e"),
                 (40, 20, 100000, "h")]
    return sc


def _tandem():
    """seeds beside and inside a tandem of period 2 and one of period 1: the
    matches on every second (every) diagonal pay for ever more indels, and
    the band passes 16, 32 and 64 diagonals"""
    sc = Scenario("tandem", 2400, 45)
    t = sc.text
    for at, m, period in ((200, 60, 2), (500, 120, 2), (900, 400, 2),
                          (1500, 300, 1)):
        t[at:at + m] = np.tile(t[at:at + period], m // period)
        t[at - 1] = (int(t[at + period - 1]) + 1) % 4
        # a read that ends in / begins with the tandem, the seed in the flank
        sc.planted(at - 40, 20, 12, m + 8, [(4, "s")], [], beside=False)
        sc.planted(at + m - 20, m + 8, 12, 20, [], [(4, "s")], beside=False)
        # seeds of the text against itself inside it
        for dist in (period, 3 * period):
            sc_self = (at + 4, at + 4 + dist, 10)
            sc.selfpairs = getattr(sc, "selfpairs", []) + [sc_self]
    sc.params = [(20, 5, 100000, "e"), (20, 20, 100000, "e"),
                 (20, 60, 100000, "e"), (20, 20, 100000, "h")]
    return sc


def _tandemself():
    """the repeats of the tandems of `tandem` against themselves"""
    src = _tandem()
    sc = Scenario("tandemself", 2400, 45)
    sc.text = src.text
    for a, b, s in src.selfpairs:
        sc.selfseed(a, b, s)
        sc.selfseed(b, a, s)
    sc.params = [(12, 5, 100000, "he"), (12, 20, 100000, "he")]
    return sc


def _mirrored():
    """reads whose seeds lie 3 .. 10 symbols behind their start, with an
    indel or two between the seed and that start: a diagonal of a left
    generation reads the separator in front of the read and shortens vlen,
    and a higher diagonal of the SAME generation then slides under the new
    length, where the same J addresses another symbol (vseq[vlen - 1 - J])"""
    sc = Scenario("mirrored", 1200, 130)
    for w in range(100, 400, 40):
        for a in (3, 4, 5, 6, 7, 8, 10):
            for le in ([(1, "i")], [(2, "i")], [(1, "d")], [(2, "d")],
                       [(1, "i"), (3, "i")], [(1, "d"), (3, "d")]):
                sc.planted(w, a, 10, 6, le, [])
    sc.params = [(10, 5, 100000, "e"), (10, 20, 100000, "e"),
                 (10, 2, 100000, "e")]
    return sc


def _ties():
    """a run of one symbol and then X Y X Y .. in the text against Y X Y X ..
    in the read: diagonals -1 and +1 of generation 1 slide equally far and
    reach the same score, above the best of generation 0 -- the lower one is
    kept, and the two would give other lengths; the same to the left; and
    the run alone, where generation 1 only equals the best of generation 0"""
    sc = Scenario("ties", 600, 47)
    t = sc.text
    for w, m in ((100, 6), (300, 3)):
        t[w + 20:w + 30] = 0
        t[w + 19] = 3
        t[w + 30:w + 30 + 2 * m] = np.tile([1, 2], m)
        t[w + 30 + 2 * m] = 3
        q = t[w:w + 60].copy()
        q[30:30 + 2 * m] = np.tile([2, 1], m)
        q[30 + 2 * m:] = (q[30 + 2 * m:] + 1) % 4
        sc.reads.append(q)
        sc.seed(len(sc.reads) - 1, 8, 12, w + 8)
        # ... mirrored: the seed behind the run
        t[w + 100:w + 100 + 2 * m] = np.tile([1, 2], m)
        t[w + 99] = 3
        t[w + 100 + 2 * m:w + 110 + 2 * m] = 0
        t[w + 110 + 2 * m] = 3
        q = t[w + 80:w + 140].copy()
        q[20:20 + 2 * m] = np.tile([2, 1], m)
        q[:20] = (q[:20] + 1) % 4
        sc.reads.append(q)
        sc.seed(len(sc.reads) - 1, 31 + 2 * m, 12, w + 111 + 2 * m)
    sc.params = [(14, 5, 100000, "he"), (14, 20, 100000, "e"),
                 (14, 2, 100000, "e")]
    return sc


def scenarios(lane_budget, long_step):
    """name -> Scenario; the limits are the ones the library exports"""
    out = [
        adopt(DC._borders(False), "borders",
              [(6, 1, 4, "he"), (10, 2, 4, "he"), (10, 5, 4, "he"),
               (8, 20, 4, "he"), (8, 255, 4, "he")]),
        adopt(DC._borders(True), "borders_dense",
              [(6, 1, 5, "he"), (10, 3, 5, "he"), (12, 20, 5, "he")]),
        adopt(DC._bothempty(), "bothempty", [(10, 2, 12, "he")]),
        _drops(), _hspecials(),
        adopt(DC._indels(), "indels",
              [(20, 1, 10, "e"), (20, 2, 10, "e"), (20, 3, 10, "he"),
               (30, 20, 10, "he")]),
        adopt(DC._selfseeds(), "selfseeds",
              [(12, 2, 8, "he"), (16, 5, 8, "he"), (12, 20, 9, "he")]),
        _slides(lane_budget, long_step), _manygenerations(), _tandem(),
        _tandemself(), _mirrored(), _ties()]
    return {sc.name: sc for sc in out}


SCENARIOS = ("borders", "borders_dense", "bothempty", "drops", "hspecials",
             "indels", "selfseeds", "slides", "manygenerations", "tandem",
             "tandemself", "mirrored", "ties")


def modes(sc):
    """[(L, X, S, hamming)] of a scenario"""
    return [(L, X, S, m == "h") for L, X, S, ms in sc.params for m in ms]
