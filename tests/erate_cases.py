"""The recorded runs of vmatch -pp matchcluster erate E
(tests/golden/matchcluster_erate_manifest.json and
matchcluster_erate_expected.npz, written by scripts/make_golden_matchcluster_erate.py): the recipes from which
both the vmatch command line and the calls of the library are derived.  All
runs are self lists (-l L) on the index of tests/golden/at1MB.gz; the lists of
-l 60, 30 and 20 are those the gapsize and overlap runs store
(matchcluster_expected.npz), that of -l 100 is stored here.  Shared by the
generator and the two erate test modules."""
import json
import os

import numpy as np

import helpers as H
import cluster_cases as CC
import matchcluster_cases as MC
import erate_model as EM

md5 = CC.md5


def R(key, L, erate, matches, edges, clusters, largest):
    return dict(key=key, L=L, erate=erate, matches=matches, edges=edges,
                clusters=clusters, largest=largest)


# largest: the largest distance of an edge
RUNS = [
    R("l60_erate5", 60, 5, 1330, 10132, 144, 15),
    R("l60_erate0", 60, 0, 1330, 8735, 151, 0),
    R("l30_erate10", 30, 10, 3012, 33706, 264, 27),
    R("l100_erate20", 100, 20, 470, 2032, 40, 56),
    R("l20_erate10", 20, 10, 4507, 41982, 444, 27),
]
# runs whose edges are left out of the archive: the counts and md5s stay
NOEDGES = ("l30_erate10", "l20_erate10")
# lists the other archive does not hold
OWNLISTS = (100,)


def run_of(key):
    return next(r for r in RUNS if r["key"] == key)


def keys():
    return [r["key"] for r in RUNS]


def list_args(r):
    return ["-l", str(r["L"])]


def cluster_args(r, prefix):
    return ["-pp", "matchcluster", "erate", str(r["erate"]), "outprefix",
            prefix]


def text():
    """the symbols of at1MB with separators"""
    return CC.text()[0]


def layout_kwargs(r, **more):
    return CC.layout_kwargs(r, **more)


_manifest = None
_arrays = None


def manifest():
    global _manifest
    if _manifest is None:
        with open(os.path.join(H.GOLDEN,
                               "matchcluster_erate_manifest.json")) as f:
            _manifest = json.load(f)
    return _manifest


def array(name):
    global _arrays
    if _arrays is None:
        _arrays = np.load(os.path.join(H.GOLDEN,
                                       "matchcluster_erate_expected.npz"))
    return _arrays[name]


def input_of(key):
    """the records of the list the clusterer of a run sees"""
    L = run_of(key)["L"]
    rows = array("l%d__in" % L) if L in OWNLISTS else MC.array("l%d__in" % L)
    rec, flags = CC.records_of(rows)
    assert not flags.any()
    return rec


def view(rec):
    """-> (length, position1, position2) as lists of int"""
    return ([int(x) for x in rec["length"]], [int(x) for x in rec["dbstart"]],
            [int(x) for x in rec["queryseq"]])


def model_of(r, rec, **kw):
    return EM.cluster(text(), *view(rec), r["erate"], **kw)


def sink_of(V, r):
    s = V.Sink(**layout_kwargs(r))
    s.setdigits()
    return s


def text_of(got, lines):
    """cluster c of `got` (members, edges and values as arrays) -> the bytes
    of its file behind its first line, from the line of every record"""
    def text(c):
        a, b = (int(x) for x in got["clusterstart"][c:c + 2])
        e0, e1 = (int(x) for x in got["edgestart"][c:c + 2])
        mem = [int(m) for m in got["members"][a:b]]
        return EM.format_cluster(
            mem, [lines[m] for m in mem],
            list(zip(got["m0"][e0:e1].tolist(), got["m1"][e0:e1].tolist(),
                     np.asarray(got["values"][e0:e1], np.uint64).tolist())))
    return text


def check_against_manifest(key, got, cluster_text):
    """got: a dict like EM.cluster returns (stats as a dict); cluster_text(c)
    -> the bytes of the file of cluster c behind its first line"""
    e = manifest()[key]
    for k in ("matches", "candidates", "samematch", "below", "edges",
              "forestedges", "clusters", "inclusters"):
        assert got["stats"][k] == e["stats"][k], k
    assert md5(got["text"]) == e["md5_text"]
    assert np.array_equal(got["clusterstart"], array(key + "__clusterstart"))
    assert np.array_equal(got["members"], array(key + "__members"))
    assert np.array_equal(got["edgestart"], array(key + "__edgestart"))
    if key + "__m0" in e["stored"]:
        assert np.array_equal(got["m0"], array(key + "__m0"))
        assert np.array_equal(got["m1"], array(key + "__m1"))
        assert np.array_equal(got["values"], array(key + "__values"))
    assert len(e["md5_files"]) == e["stats"]["clusters"]
    for c, want in enumerate(e["md5_files"]):
        assert md5(cluster_text(c)) == want, (key, c)


# --------------------------------------------------------------------------
# hand-made texts and lists: a text is built from segments, every segment
# followed by ten random symbols, so that no two instances touch
# --------------------------------------------------------------------------

class Text:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.parts, self.n = [], 0

    def random(self, length):
        return self.rng.integers(0, 4, length).astype(np.uint8)

    def put(self, symbols, gap=10):
        """-> the position of the segment"""
        at = self.n
        seg = np.asarray(symbols, np.uint8)
        self.parts += [seg, self.random(gap)]
        self.n += len(seg) + gap
        return at

    def symbols(self):
        return np.concatenate(self.parts)


def substituted(seq, d, shift=0):
    """d substitutions, evenly spread"""
    out = np.array(seq, np.uint8)
    for x in range(d):
        at = ((2 * x + 1) * len(seq)) // (2 * d) + shift
        out[at] = (out[at] + 1) % 4
    return out


def records(length, position1, position2):
    return MC.records(length, position1, position2)


def layout_of(V, text):
    return V.sink_params(kind=2, totallength=len(text),
                         markpos=np.flatnonzero(text == H.SEPARATOR)
                         .astype(np.uint64))


def edited(seq, d, fill):
    """d edit operations, the result as long as seq: from a bound of 8 on,
    g = min(3, d // 4) symbols deleted near the start and g symbols of
    `fill` inserted near the end -- between them the shortest script runs g
    diagonals off the main one, across the lanes of a group -- and d - 2 g
    substitutions between them; below that, d substitutions"""
    g = min(3, d // 4) if d >= 8 else 0
    if g == 0:
        return substituted(seq, d)
    seq = np.asarray(seq, np.uint8)
    cut, at = len(seq) // 20, len(seq) - len(seq) // 20
    # (the substitutions keep clear of the symbols deleted and inserted)
    mid = substituted(seq[cut + g + 2:at - g - 2], d - 2 * g)
    if d % 2 == 1:
        # an odd d the other way round: inserted first, deleted last, the
        # diagonals above the main one
        return np.concatenate([seq[:cut], fill[:g], seq[cut:cut + g + 2], mid,
                               seq[at - g - 2:at - g], seq[at:]])
    return np.concatenate([seq[:cut], seq[cut + g:cut + g + 2], mid,
                           seq[at - g - 2:at], fill[:g], seq[at:]])


def bound_case(t, maxdist):
    """three matches on the Text t whose bound is exactly `maxdist` under
    E = 10: match 1 is match 0 after maxdist edit operations (edited), match
    2 after maxdist + 1 -> records.  Random symbols can make a script one
    operation cheaper than it was built: the inserted symbols are drawn again
    until the model says maxdist for the one and more for the other."""
    L = 10 * maxdist + 3
    a = t.random(L)
    for attempt in range(50):
        near, far = edited(a, maxdist, t.random(3)), \
            edited(a, maxdist + 1, t.random(3))
        both = np.concatenate([a, near, far])
        if EM.front_answer(both, 0, L, L, L, maxdist) == maxdist and \
                EM.front_answer(both, 0, L, 2 * L, L, maxdist) == -1:
            break
    else:
        raise AssertionError("no bound case for %d" % maxdist)
    assert len(near) == len(far) == L
    pos = [t.put(s) for s in (a, a, near, near, far, far)]
    return records(L, pos[0::2], pos[1::2])


def planted_list(seed, n=36, families=5):
    """a random text with wildcards and families of near-copies, and a list
    of n matches whose instances are such copies, whole or in part, some of
    them overlapping in the text -> (text, records)"""
    t = Text(seed)
    rng = t.rng
    starts = []
    for f in range(families):
        base = t.random(70)
        if f == 0:
            base[33] = H.WILDCARD
        for c in range(4):
            copy = substituted(base, int(rng.integers(0, 5)),
                               int(rng.integers(0, 3)))
            if c == 3:
                copy = np.delete(copy, int(rng.integers(5, 60)))
            starts.append(t.put(copy))
    length = rng.integers(20, 61, n)
    p1 = rng.choice(starts, n) + rng.integers(0, 4, n)
    p2 = rng.choice(starts, n) + rng.integers(0, 4, n)
    return t.symbols(), records(length, p1, p2)
