"""The X-drop extension of exact seeds on the host (vmatch -l L -hxdrop X |
-exdrop X): vsa_extend_xdrop_host, fed with the seed lists of the CPU oracle,
against every recorded run of the real reference (tests/golden/extend_xdrop_*),
row for row and in order, and the lines of the sink against the recorded md5;
the literal Python model (extend_xdrop_model.py) against the host code on
parts of the same seed lists and on the hand-made border cases, at 1 and 4
threads and with one symbol per step; the reference's error for X = 256; the
host code also as a program of its own under the sanitizers.  No GPU.

The model reproduced every recorded list in full when the fixtures were
written (scripts/make_golden_extend_xdrop.py writes nothing otherwise).  Here
it goes through a part of the seeds of a run -- the longest ones and every
n-th of the others; every seed is extended on its own, so host code and model
must agree on any part of a list."""
import os
import re
import subprocess

import numpy as np
import pytest

import extend_xdrop_cases as XC
import extend_xdrop_model as XM
import helpers as H

# seeds of a run the model goes through (it takes milliseconds per seed, but
# seconds for a seed inside a repeat of thousands of symbols)
MODEL_SEEDS = 150
# ... and the longest match the model is asked for
MODEL_MAXLENGTH = 600

_seeds = {}


def seeds_of(key):
    """[(palindromic, batch or None, seed list of the oracle)] of a run"""
    if key not in _seeds:
        r = XC.run_of(key)
        _seeds[key] = [(pal, q, XC.oracle_seeds(r, q))
                       for pal, q in XC.passes(r)]
    return _seeds[key]


def triple(q):
    return None if q is None else (q.symbols, q.start, q.length)


@pytest.mark.parametrize("key", XC.golden_keys())
def test_host_code_equals_every_recorded_list_and_the_model(V, key):
    r, e = XC.run_of(key), XC.manifest()[key]
    idx, _ = XC.load(r)
    want = XC.expected_rows(key)
    assert len(want) == e["lines"]
    host, text, nseeds = [], [], 0
    for pal, q, seeds in seeds_of(key):
        nseeds += len(seeds)
        got = V.extend_xdrop_host(idx.tis, seeds, r["L"], r["X"], r["S"],
                                  queries=triple(q),
                                  numofchars=idx.numofchars, threads=3,
                                  hamming=r["hamming"])
        host.append(XC.rows_of(r, got, pal))
        text.append(V.Sink(**XC.sink_kwargs(V, r, pal)).format(got))
        # a part of the list through the model: every n-th seed
        part = seeds[::max(1, len(seeds) // MODEL_SEEDS)]
        if e["maxlength"] > MODEL_MAXLENGTH:
            part = part[:4]
        rec = XM.extend(part, idx.tis, r["L"], r["X"], r["hamming"], r["S"],
                        triple(q))
        got = V.extend_xdrop_host(idx.tis, part, r["L"], r["X"], r["S"],
                                  queries=triple(q),
                                  numofchars=idx.numofchars, threads=1,
                                  hamming=r["hamming"])
        assert np.array_equal(got, rec)
    assert nseeds == e["seeds"]
    assert np.array_equal(np.concatenate(host), want)
    assert int(np.abs(want[:, 6]).max()) == e["maxdistance"]
    assert (want[:, 6] <= 0).all() if r["hamming"] else (want[:, 6] >= 0).all()
    assert int((want[:, 0] != want[:, 3]).sum()) == e["unequal"]
    assert XC.md5(b"".join(text)) == e["md5_lines"]


def test_the_recorded_runs_are_the_ones_the_issue_names():
    m = XC.manifest()
    assert set(m) == {r["key"] for r in XC.RUNS} and len(m) == 24
    good = [m[k] for k in XC.golden_keys()]
    cases = {(e["case"], e["q"]) for e in good}
    assert cases == {("c5", True), ("at1mb", False), ("grumbach", True),
                     ("grumbach_all", False), ("micro", True),
                     ("wildcards", True), ("wildcards", False),
                     ("prot", True), ("prot", False), ("largepat", False)}
    assert {e["X"] for e in good} == {1, 2, 5, 20, 255}
    assert {bool(e["S"]) for e in good} == {True, False}
    assert any(e["strands"] == "dp" for e in good)
    for e in good:
        assert 0 < e["lines"] <= 6000
        assert e["args"][e["args"].index("-l") + 2] == \
            ("-hxdrop" if e["hamming"] else "-exdrop")
        assert e["hamming"] == (e["unequal"] == 0) or not e["hamming"]
    # unequal lengths; fewer lines than seeds by the reject rule or the
    # least length; a left side that reads a separator behind its first
    # symbol; bands the widest group of the device does not hold
    assert any(not e["hamming"] and e["unequal"] > 0 for e in good)
    assert any(e["hamming"] and e["lines"] < e["seeds"] for e in good)
    assert any(not e["hamming"] and e["sepreads"] > 0 for e in good)
    assert any(not e["hamming"] and e["maxwidth"] > 64 for e in good)
    assert max(e["maxdistance"] for e in good) > 0xFFFF
    for name in ("extend_xdrop_manifest.json", "extend_xdrop_expected.npz"):
        assert os.path.getsize(os.path.join(H.GOLDEN, name)) <= 400 * 1024


def test_the_recorded_error(V):
    """X = 256: what the reference says, recorded verbatim, and what the
    host entry says of the same bound"""
    r = XC.run_of("c5_q_l40_hx256")
    assert XC.manifest()[r["key"]]["stderr"] == \
        'argument "256" to option -hxdrop must be in the range [1,255]'
    idx, q = XC.load(r)
    seeds = H.oracle_querymatches(idx, q, 30, speedup=2)[:5]
    with pytest.raises(V.VsaError) as e:
        V.extend_xdrop_host(idx.tis, seeds, r["L"], r["X"], queries=triple(q),
                            hamming=True)
    assert e.value.code == -2 and e.value.message == \
        "vsa_extend_xdrop_host: X = 256: the reference takes 1 to 255 " \
        "(FLAGXDROP, Vmatch/parsevm.c)"
    assert V.XDROP_MAXDROP == 255


SC = XC.scenarios(256, 1024)
_models = {}


def model(sc, L, X, S, hamming):
    k = (sc.name, L, X, S, hamming)
    if k not in _models:
        _models[k] = sc.model(L, X, S, hamming)
        _models[k].setflags(write=False)
    return _models[k]


def test_the_limits_the_scenarios_are_built_around(V):
    assert V.EXTEND_LANE_BUDGET == 256 and V.EXTEND_LONG_STEP == 1024
    assert V.extend_xdrop_seedlength() == 30 == XM.seedlength_rule()
    assert V.extend_xdrop_seedlength(7) == 7 == XM.seedlength_rule(7)
    assert set(SC) == set(XC.SCENARIOS)
    for sc in SC.values():
        assert len(sc.text) <= 4096 and len(sc.seeds) <= 1024
    # the record, each way
    rec = np.zeros(3, V.MATCH_DTYPE)
    rec["length"] = [5 | 7 << 32, 0xFFFFFFEF | 0xFFFFFFEF << 32, 300]
    rec["querystart"] = [9 | 70000 << 32, 0xFFFFFFEF << 32, 17]
    for a, b in ((V.xdrop_lengths1, XM.lengths1),
                 (V.xdrop_lengths2, XM.lengths2),
                 (V.xdrop_starts, XM.starts),
                 (V.xdrop_distances, XM.distances)):
        assert np.array_equal(a(rec), b(rec))
    assert list(V.xdrop_lengths2(rec)) == [7, 0xFFFFFFEF, 0]
    assert list(V.xdrop_distances(rec)) == [70000, 0xFFFFFFEF, 0]
    assert XM.pack(5, 7, 9, -70000) == (int(rec["length"][0]),
                                        int(rec["querystart"][0]))


@pytest.mark.parametrize("name", XC.SCENARIOS)
def test_host_code_equals_the_model_on_the_border_cases(V, name, monkeypatch):
    sc = SC[name]
    seeds = sc.records()
    some = 0
    for L, X, S, hamming in XC.modes(sc):
        want = model(sc, L, X, S, hamming)
        for threads in (1, 4):
            got = V.extend_xdrop_host(sc.text, seeds, L, X, S,
                                      queries=sc.triple(), threads=threads,
                                      hamming=hamming)
            assert np.array_equal(got, want), (L, X, S, hamming)
        # one symbol per step
        monkeypatch.setenv("VSA_EXTEND_XDROP_SCALAR", "1")
        got = V.extend_xdrop_host(sc.text, seeds, L, X, S,
                                  queries=sc.triple(), threads=2,
                                  hamming=hamming)
        monkeypatch.delenv("VSA_EXTEND_XDROP_SCALAR")
        assert np.array_equal(got, want), (L, X, S, hamming)
        some += len(want)
    assert some > 0
    # a list in which every seed is dropped, and an empty list
    for hamming in (True, False):
        assert len(V.extend_xdrop_host(sc.text, seeds, 100000, 2,
                                       queries=sc.triple(),
                                       hamming=hamming)) == 0
        assert len(V.extend_xdrop_host(sc.text, seeds[:0], 20, 2,
                                       queries=sc.triple(),
                                       hamming=hamming)) == 0


def test_ties_and_equal_predecessors_occur_in_the_scenarios():
    """what pins the comparisons of the rules: generations in which two
    diagonals reach the best score of the side (the lowest one is kept), a
    later generation that only equals the best (the earlier one stays), and
    entries whose predecessors offer the same row (insertion `<`, mismatch
    and deletion `<=`).  Counted by a model that watches for them; the lists
    of these scenarios are compared with host code and kernels."""
    seen = {"lanes": 0, "generations": 0, "predecessors": 0}
    from extend_model import multiseq
    for name in ("ties", "indels", "drops"):
        sc = SC[name]
        seq1 = [int(c) for c in sc.text]
        seq2, qstart = multiseq(*sc.triple())
        for m in sc.records()[:40]:
            p1 = int(m["dbstart"])
            p2 = qstart[int(m["queryseq"])] + int(m["querystart"])
            e = p1 + int(m["length"])
            f = p2 + int(m["length"])
            if e >= len(seq1) or f >= len(seq2) or \
                    XM.SEPARATOR in (seq1[e], seq2[f]):
                continue
            for k, v in ties_of_a_right_side(seq1, e, seq2, f, 5).items():
                seen[k] += v
    assert all(v > 0 for v in seen.values()), seen
    # the tie of two lanes decides the lengths of a match
    sc = SC["ties"]
    want = model(sc, 14, 5, 100000, False)
    assert (XM.lengths1(want) != XM.lengths2(want)).any()


def ties_of_a_right_side(seq1, uoff, seq2, voff, X):
    """EVALXDROPEDITRIGHT once more, without pruning details left out, only
    to COUNT: equal maxima within a generation, a generation that equals
    the best of an earlier one, equal predecessors"""
    out = {"lanes": 0, "generations": 0, "predecessors": 0}
    rows = {}

    def watch(best, scores):
        top = max(scores) if scores else None
        if top is not None and scores.count(top) > 1 and top > best:
            out["lanes"] += 1
        if top is not None and top == best:
            out["generations"] += 1

    # the model with a hook: the rows of every generation
    trace = {}
    XM.evalxdropedit(False, seq1, uoff, len(seq1) - uoff, seq2, voff,
                     len(seq2) - voff, X, trace=trace, rows=rows)
    best = None
    for d in sorted(rows):
        smallest, row, dmulti, prevbest = rows[d]
        scores = [2 * i - (smallest + n) - dmulti
                  for n, i in enumerate(row) if i is not None]
        if d > 0:
            watch(prevbest, scores)
            prev = rows[d - 1]
            for n in range(len(row)):
                k = smallest + n
                at = k - prev[0]
                cand = []
                for off, add in ((1, 0), (0, 1), (-1, 1)):
                    if 0 <= at + off < len(prev[1]) and \
                            prev[1][at + off] is not None:
                        cand.append(prev[1][at + off] + add)
                if len(cand) > 1 and cand.count(max(cand)) > 1:
                    out["predecessors"] += 1
    return out


def test_matches_depend_on_the_mutable_lengths_and_their_order(V):
    """the scenario `mirrored`: left sides whose result depends on ulen / vlen
    being state and on the order of the diagonals within a generation.  The
    model with the lengths frozen and the model with every diagonal under the
    lengths of the start of its generation each give another result or none;
    the host code gives the literal model's, which is the reference's"""
    sc = SC["mirrored"]
    L, X, S, _ = sc.params[0]
    recs = sc.records()
    literal = XM.matches(recs, sc.text, X, False, S, sc.triple())[0]
    frozen = XM.matches(recs, sc.text, X, False, S, sc.triple(),
                        frozen=True)[0]
    unordered = XM.matches(recs, sc.text, X, False, S, sc.triple(),
                           unordered=True)[0]
    both = [i for i in range(len(recs))
            if literal[i] != frozen[i] and literal[i] != unordered[i]]
    assert len(both) >= 3
    for i in both[:5]:
        want = XM.extend(recs[i:i + 1], sc.text, 1, X, False, S, sc.triple())
        got = V.extend_xdrop_host(sc.text, recs[i:i + 1], 1, X, S,
                                  queries=sc.triple(), hamming=False)
        assert len(want) == 1 and np.array_equal(got, want)


def test_host_code_refuses_what_does_not_fit(V):
    sc = SC["borders"]
    q, seeds = sc.queries(), sc.records()
    for field, value in (("dbstart", len(sc.text)), ("queryseq", q.nq),
                         ("querystart", 1 << 20), ("length", 0),
                         ("length", 1 << 50)):
        bad = seeds.copy()
        bad[field][5] = value
        with pytest.raises(V.VsaError) as e:
            V.extend_xdrop_host(sc.text, bad, 10, 2, queries=sc.triple(),
                                hamming=False)
        assert e.value.code == -2 and "record 5 does not fit" in \
            e.value.message
    for L, X in ((0, 2), (10, 0), (10, 256)):
        with pytest.raises(V.VsaError) as e:
            V.extend_xdrop_host(sc.text, seeds, L, X, queries=sc.triple(),
                                hamming=True)
        assert e.value.code == -2
    # the wrappers need the flag of the kind, and only that
    with pytest.raises(TypeError):
        V.extend_xdrop_host(sc.text, seeds, 10, 2, queries=sc.triple())
    with pytest.raises(TypeError):
        V.extend_hamming_host(sc.text, seeds, 10, 2, queries=sc.triple(),
                              hamming=True)


def test_every_entry_of_the_header_has_its_mirror(V):
    text = open(os.path.join(H.ROOT, "include", "vstree_amd_xdrop.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(vsa_[a-z0-9_]+)\s*\(", text)))
    assert len(syms) == 5 and syms == V.XDROP_ABI_SYMBOLS
    out = subprocess.check_output(["nm", "-D", "--defined-only",
                                   V.LIBPATH_NORT]).decode()
    have = {l.split()[-1] for l in out.splitlines() if l}
    assert set(syms) <= have
    # what the kernels ask of the host unit beside the entry is no export
    assert "vsa_xd_host_seeds" not in have
    assert (V.SINK_QUERY_HXDROP, V.SINK_SELF_HXDROP, V.SINK_QUERY_EXDROP,
            V.SINK_SELF_EXDROP) == (12, 13, 14, 15)
    main = open(os.path.join(H.ROOT, "include", "vstree_amd.h")).read()
    for name, value in (("VSA_SINK_QUERY_HXDROP", 12),
                        ("VSA_SINK_SELF_HXDROP", 13),
                        ("VSA_SINK_QUERY_EXDROP", 14),
                        ("VSA_SINK_SELF_EXDROP", 15),
                        ("VSA_XDROP_MAXDROP", "255u")):
        assert re.search(r"#define %s\s+%s\b" % (name, value), main)


def test_handles_refuse_layouts_of_extended_seeds(V):
    rec = np.zeros(2, V.MATCH_DTYPE)
    rec["length"] = 20
    for kind in (V.SINK_QUERY_HXDROP, V.SINK_SELF_HXDROP,
                 V.SINK_QUERY_EXDROP, V.SINK_SELF_EXDROP):
        lay = V.sink_params(kind=kind, totallength=1000, markpos=[])
        for call in (lambda: V.select_host(lay, rec),
                     lambda: V.chain_host(lay, rec)):
            with pytest.raises(V.VsaError) as e:
                call()
            assert e.value.code == V.NOT_COVERED
            assert "extended seeds" in e.value.message


def test_host_code_under_the_sanitizers_as_a_program_of_its_own(tmp_path):
    """extend_xdrop_host.c with the rules and
    scripts/extend_xdrop_host_check.c built with -fsanitize=address,undefined:
    the border cases, eight symbols per step against one, no Python and no
    GPU in the process"""
    exe = str(tmp_path / "extend_xdrop_host_check")
    csrc = os.path.join(H.ROOT, "vstree_amd", "csrc")
    subprocess.check_call(
        ["gcc", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-Wall", "-Wextra",
         "-Wno-format-truncation",
         "-I" + os.path.join(H.ROOT, "include"), "-I" + csrc,
         os.path.join(H.ROOT, "scripts", "extend_xdrop_host_check.c"),
         os.path.join(csrc, "extend_xdrop_host.c"), "-o", exe, "-lm",
         "-lpthread"])

    def run(sc, seeds, L, X, hamming, S, threads):
        q = sc.queries()
        path = str(tmp_path / "seeds.txt")
        with open(path, "w") as f:
            sym = q.symbols if q is not None else np.zeros(0, np.uint8)
            nq = q.nq if q is not None else 0
            f.write("%d %d %d %d %d %d %d %d %d\n" % (
                len(sc.text), len(sym), nq, len(seeds), L, X, int(hamming), S,
                threads))
            f.write(" ".join(str(int(c)) for c in sc.text) + "\n")
            f.write(" ".join(str(int(c)) for c in sym) + "\n")
            for i in range(nq):
                f.write("%d %d\n" % (q.start[i], q.length[i]))
            for x in seeds:
                f.write("%d %d %d %d\n" % tuple(int(v) for v in x))
        return subprocess.run([exe, path], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE)

    for name in XC.SCENARIOS:
        sc = SC[name]
        L, X, S, hamming = XC.modes(sc)[-1]
        p = run(sc, sc.records(), L, X, hamming, S, 2)
        assert p.returncode == 0, p.stderr.decode()
        assert b"Sanitizer" not in p.stderr and b"runtime error" not in \
            p.stderr
        want = model(sc, L, X, S, hamming)
        got = np.array([[int(v) for v in l.split()]
                        for l in p.stdout.decode().splitlines()],
                       np.int64).reshape(-1, 6)
        assert np.array_equal(got[:, 0], XM.lengths1(want).astype(np.int64))
        assert np.array_equal(got[:, 1], XM.lengths2(want).astype(np.int64))
        assert np.array_equal(got[:, 2], XM.distances(want).astype(np.int64))
        assert np.array_equal(got[:, 3], want["dbstart"].astype(np.int64))
        assert np.array_equal(got[:, 4], want["queryseq"].astype(np.int64))
        assert np.array_equal(got[:, 5], XM.starts(want).astype(np.int64))
    sc = SC["borders"]
    bad = sc.records()
    bad["querystart"][3] = 1 << 30
    p = run(sc, bad, 10, 2, False, 0, 1)
    assert p.returncode == 1 and b"record 3 does not fit" in p.stderr
    assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr
