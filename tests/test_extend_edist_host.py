"""The edit-distance extension of exact seeds on the host (vmatch -l L -e K
outside -complete): vsa_extend_edist_host, fed with the seed lists of the CPU
oracle, against every recorded run of the real reference
(tests/golden/extend_edist_*), row for row and in order, and the lines of the
sink against the recorded md5; the literal Python model
(extend_edist_model.py) against the host code on the same seed lists; the
reference's error; the hand-made border cases, model against host code, the
host code also as a program of its own under the sanitizers.  No GPU.

The model reproduced every recorded list in full when the fixtures were
written (scripts/make_golden_extend_edist.py writes nothing otherwise).  Here
it goes through whole lists where that takes a few seconds, and through a
part of the seeds -- the longest ones and every n-th of the others -- of the
three runs with 10^5 seeds and more or with K = 20; every seed is extended on
its own, so host code and model must agree on any part of a list."""
import os
import re
import subprocess

import numpy as np
import pytest

import extend_edist_cases as DC
import extend_edist_model as DM
import extend_model as EM
import helpers as H

# front entries the model evaluates per run at most: seeds * 2 (K + 1)^2
MODEL_ENTRIES = 300000

_seeds = {}


def seeds_of(key):
    """[(palindromic, batch or None, seed list of the oracle)] of a run"""
    if key not in _seeds:
        r = DC.run_of(key)
        _seeds[key] = [(pal, q, DC.oracle_seeds(r, q))
                       for pal, q in DC.passes(r)]
    return _seeds[key]


def triple(q):
    return None if q is None else (q.symbols, q.start, q.length)


def part_for_the_model(seeds, K, npasses):
    cap = MODEL_ENTRIES // (2 * (K + 1) ** 2 * npasses)
    if len(seeds) <= cap:
        return seeds
    longest = np.argsort(-seeds["length"].astype(np.int64),
                         kind="stable")[:cap // 2]
    every = np.arange(0, len(seeds), max(1, 2 * len(seeds) // cap))
    return seeds[np.union1d(longest, every)]


@pytest.mark.parametrize("key", DC.golden_keys())
def test_host_code_equals_every_recorded_list_and_the_model(V, key):
    r, e = DC.run_of(key), DC.manifest()[key]
    idx, _ = DC.load(r)
    want = DC.expected_rows(key)
    assert len(want) == e["lines"]
    host, text = [], []
    for pal, q, seeds in seeds_of(key):
        got = V.extend_edist_host(idx.tis, seeds, r["L"], r["K"], r["S"],
                                  queries=triple(q),
                                  numofchars=idx.numofchars, threads=3)
        host.append(DC.rows_of(r, got, pal))
        text.append(V.Sink(**DC.sink_kwargs(V, r, pal)).format(got))
        part = part_for_the_model(seeds, r["K"], len(seeds_of(key)))
        rec = DM.extend(part, idx.tis, idx.numofchars, r["L"], r["K"],
                        r["S"], triple(q))
        if part is not seeds:
            got = V.extend_edist_host(idx.tis, part, r["L"], r["K"], r["S"],
                                      queries=triple(q),
                                      numofchars=idx.numofchars, threads=1)
        assert np.array_equal(got, rec)
    assert np.array_equal(np.concatenate(host), want)
    assert int(want[:, 6].max()) == e["maxdistance"] <= r["K"]
    assert int((want[:, 0] != want[:, 3]).sum()) == e["unequal"] > 0
    assert DC.md5(b"".join(text)) == e["md5_lines"]


def test_the_recorded_runs_are_the_ones_the_issue_names():
    m = DC.manifest()
    assert set(m) == {r["key"] for r in DC.RUNS} and len(m) == 13
    lines = {"c5_q_l40_e2": 5385, "c5_q_l40_e2_s20": 4981,
             "at1mb_l60_e3": 3962, "at1mb_l100_e8": 5080,
             "grumbach_q_l30_e2_dp": 95, "micro_q_l8_e1": 21,
             "wildcards_q_l8_e1": 8, "wildcards_l6_e2": 42,
             "prot_l12_e2": 3230, "prot_q_l12_e2": 5676,
             "ychr3_l200_e20": 56}
    for key in DC.golden_keys():
        assert 0 < m[key]["lines"] <= 6000
        assert m[key]["args"][m[key]["args"].index("-l") + 2] == "-e"
        assert key == "grumbach_all_l30_e2" or m[key]["lines"] == lines[key]
    assert m["at1mb_l60_e3"]["unequal"] == 1349
    assert m["at1mb_l100_e8"]["maxdistance"] == 8
    assert m["ychr3_l200_e20"]["maxlength"] == 2312
    assert m["ychr3_l200_e20"]["maxdistance"] == 20
    for name in ("extend_edist_manifest.json", "extend_edist_expected.npz"):
        assert os.path.getsize(os.path.join(H.GOLDEN, name)) <= 400 * 1024


def test_the_recorded_error(V):
    # L / (K + 1) below the prefix length: what the reference says, which is
    # what the engine's search says for that seed length
    r = DC.run_of("c5_q_l10_e2")
    idx, q = DC.load(r)
    text = DC.manifest()[r["key"]]["stderr"]
    assert text == "searchlength=%d must be >= %d=prefixlen" % (
        V.extend_seedlength(r["L"], r["K"], r["S"]), idx.prefixlength)
    with pytest.raises(H.OracleError) as e:
        DC.oracle_seeds(r, q)
    assert str(e.value) == text


SC = DC.scenarios(256)


def test_the_limits_the_scenarios_are_built_around(V):
    assert V.EXTEND_LANE_BUDGET == 256 and V.EXTEND_EDIST_MAXDIST == 31
    assert len(DC.residues(SC["words"])) == 64
    for sc in SC.values():
        assert len(sc.text) <= 4096 and len(sc.seeds) <= 1024
    # the ties: matches longer than the E-value table, every candidate of
    # which has the E-value 0.0
    ev = EM.Evalues(4)
    ties = SC["fewerrors"].model(*DC.TIES)
    assert len(ties) >= 2 and DC.TIES in SC["fewerrors"].params
    assert int(np.minimum(DM.lengths1(ties), DM.lengths2(ties)).min()) >= 700
    assert all(DM.incgetevalue(ev, 1.0, d, n) == 0.0
               for d in range(DC.TIES[1] + 1) for n in (700, 720, 840, 900))
    # pairs of self seeds 1 .. K + 1 apart for the largest K
    gaps = {abs(int(b) - int(a)) for _, a, b, _ in SC["selfseeds"].seeds}
    assert set(range(1, max(K for _, K, _ in SC["selfseeds"].params) + 2)) \
        <= gaps
    # the record: both lengths and the distance, each way
    l1 = np.array([5, 1 << 40, 300, 17], np.uint64)
    l2 = np.array([5, (1 << 40) + 127, 172, 20], np.uint64)
    d = np.array([0, 125, 125, 3], np.uint64)
    rec = np.zeros(4, V.MATCH_DTYPE)
    rec["length"] = V.edist_pack(l1, l2, d)
    for a, b in ((V.edist_lengths1, DM.lengths1),
                 (V.edist_lengths2, DM.lengths2),
                 (V.edist_distances, DM.distances)):
        assert np.array_equal(a(rec), b(rec))
    assert np.array_equal(V.edist_lengths1(rec), l1)
    assert np.array_equal(V.edist_lengths2(rec), l2)
    assert np.array_equal(V.edist_distances(rec), d)
    assert [DM.pack(int(a), int(b), int(c)) for a, b, c in zip(l1, l2, d)] \
        == [int(x) for x in rec["length"]]


@pytest.mark.parametrize("name", DC.SCENARIOS)
def test_host_code_equals_the_model_on_the_border_cases(V, name,
                                                        monkeypatch):
    sc = SC[name]
    seeds = sc.records()
    some = 0
    for L, K, S in sc.params + [(30, 40, 0)]:
        want = sc.model(L, K, S)
        for threads in (1, 4):
            got = V.extend_edist_host(sc.text, seeds, L, K, S,
                                      queries=sc.triple(), threads=threads)
            assert np.array_equal(got, want), (L, K, S)
        # one symbol per step
        monkeypatch.setenv("VSA_EXTEND_EDIST_SCALAR", "1")
        got = V.extend_edist_host(sc.text, seeds, L, K, S,
                                  queries=sc.triple(), threads=2)
        monkeypatch.delenv("VSA_EXTEND_EDIST_SCALAR")
        assert np.array_equal(got, want), (L, K, S)
        some += len(want)
    assert some > 0
    # a list in which every seed is dropped, and an empty list
    assert len(V.extend_edist_host(sc.text, seeds, 100000, 2,
                                   queries=sc.triple())) == 0
    assert len(V.extend_edist_host(sc.text, seeds[:0], 20, 2,
                                   queries=sc.triple())) == 0


def _first_separator_right(maxdist, su, ustart, ulen, sv, vstart, vlen):
    """extendedrightSEP with the pre-scan over the whole side: the bounds
    are the first separators from the start and never move"""
    gl = DM.FrontResource()
    gl.su, gl.sv = su, sv
    gl.ubound, gl.vbound = ustart + ulen, vstart + vlen
    for i in range(ulen):
        if su[ustart + i] == DM.SEPARATOR:
            gl.ubound = ustart + i
            break
    for i in range(vlen):
        if sv[vstart + i] == DM.SEPARATOR:
            gl.vbound = vstart + i
            break
    gl.useq, gl.vseq, gl.ulen, gl.vlen = ustart, vstart, ulen, vlen
    h, specs = DM._fronts(gl, maxdist, False, 0)
    return h, specs, gl.frontspace


def _front_under_its_first_bounds(gl, prevfspec, fspec, r, backward,
                                  reachlength):
    """evalfront with every diagonal under the bounds of the start of the
    front, the tightest bounds behind it: lanes that slide at once and are
    NOT replayed in the order of the diagonals"""
    ub0, vb0 = gl.ubound, gl.vbound
    ubs, vbs, defined = [ub0], [vb0], False
    for i in range(fspec.width):
        k = fspec.left + i
        gl.ubound, gl.vbound = ub0, vb0
        v = gl.integermin
        if r <= 0 or k <= -r or k >= r:
            v = DM.evalentrybackward(gl, prevfspec, k, reachlength) \
                if backward else DM.evalentryforward(gl, prevfspec, k)
        defined = defined or v >= 0
        ubs.append(gl.ubound)
        vbs.append(gl.vbound)
        gl.frontspace.append(v)
    gl.ubound = max(ubs) if backward else min(ubs)
    gl.vbound = max(vbs) if backward else min(vbs)
    return defined


def test_matches_depend_on_the_literal_order_of_the_bounds(V, monkeypatch):
    """the two seeds of the scenario boundsorder: the literal model and the
    host code find matches that "bound = first separator of the side" and
    "every diagonal under the bounds of the start of its front" do not find
    (extend_edist_rules.h says why); the GPU test runs the same scenario, so
    the kernel's replay of the slides in the order of the diagonals is held
    by an output"""
    sc = SC["boundsorder"]
    L, K, S = sc.params[0]
    literal = sc.model(L, K, S)
    assert list(literal["queryseq"]) == [0, 2]
    assert np.array_equal(V.extend_edist_host(sc.text, sc.records(), L, K, S,
                                              queries=sc.triple()), literal)
    with monkeypatch.context() as m:
        m.setattr(DM, "extendedrightSEP", _first_separator_right)
        assert len(sc.model(L, K, S)) == 0
    with monkeypatch.context() as m:
        m.setattr(DM, "evalfront", _front_under_its_first_bounds)
        assert list(sc.model(L, K, S)["queryseq"]) == [0]
    # ... and where nothing hangs on a diagonal behind the separator, all
    # three agree
    L, K, S = sc.params[3]
    literal = sc.model(L, K, S)
    assert len(literal) == 2
    with monkeypatch.context() as m:
        m.setattr(DM, "extendedrightSEP", _first_separator_right)
        assert np.array_equal(sc.model(L, K, S), literal)
    with monkeypatch.context() as m:
        m.setattr(DM, "evalfront", _front_under_its_first_bounds)
        assert np.array_equal(sc.model(L, K, S), literal)


def test_host_code_refuses_what_does_not_fit(V):
    sc = SC["borders"]
    q, seeds = sc.queries(), sc.records()
    for field, value in (("dbstart", len(sc.text)), ("queryseq", q.nq),
                         ("querystart", 1 << 20), ("length", 0),
                         ("length", 1 << 50)):
        bad = seeds.copy()
        bad[field][5] = value
        with pytest.raises(V.VsaError) as e:
            V.extend_edist_host(sc.text, bad, 10, 2, queries=sc.triple())
        assert e.value.code == -2 and "record 5 does not fit" in \
            e.value.message
    for L, K in ((0, 2), (10, 0), (10, V.EDIST_MAXDISTANCE + 1)):
        with pytest.raises(V.VsaError) as e:
            V.extend_edist_host(sc.text, seeds, L, K, queries=sc.triple())
        assert e.value.code == -2
    assert V.EDIST_MAXDISTANCE == 125


def test_every_entry_of_the_header_has_its_mirror(V):
    text = open(os.path.join(H.ROOT, "include", "vstree_amd_edist.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(vsa_[a-z0-9_]+)\s*\(", text)))
    assert len(syms) == 5 and syms == V.EDIST_ABI_SYMBOLS
    out = subprocess.check_output(["nm", "-D", "--defined-only",
                                   V.LIBPATH_NORT]).decode()
    assert set(syms) <= {l.split()[-1] for l in out.splitlines() if l}
    assert (V.SINK_QUERY_EDIST, V.SINK_SELF_EDIST) == (10, 11)
    main = open(os.path.join(H.ROOT, "include", "vstree_amd.h")).read()
    for name, value in (("VSA_SINK_QUERY_EDIST", 10),
                        ("VSA_SINK_SELF_EDIST", 11),
                        ("VSA_EDIST_MAXDISTANCE", "125u"),
                        ("VSA_EXTEND_EDIST_MAXDIST", "31u")):
        assert re.search(r"#define %s\s+%s\b" % (name, value), main)


def test_handles_refuse_layouts_of_extended_seeds(V):
    rec = np.zeros(2, V.MATCH_DTYPE)
    rec["length"] = 20
    for kind in (V.SINK_SELF_EDIST, V.SINK_QUERY_EDIST):
        lay = V.sink_params(kind=kind, totallength=1000, markpos=[])
        for call in (lambda: V.select_host(lay, rec),
                     lambda: V.chain_host(lay, rec)):
            with pytest.raises(V.VsaError) as e:
                call()
            assert e.value.code == V.NOT_COVERED
            assert "extended seeds" in e.value.message


def test_host_code_under_the_sanitizers_as_a_program_of_its_own(tmp_path):
    """extend_edist_host.c with the rules, match_sink.c (the E-value table)
    and scripts/extend_edist_host_check.c built with
    -fsanitize=address,undefined: the border cases, eight symbols per step
    against one, no Python and no GPU in the process"""
    exe = str(tmp_path / "extend_edist_host_check")
    csrc = os.path.join(H.ROOT, "vstree_amd", "csrc")
    subprocess.check_call(
        ["gcc", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-Wall", "-Wextra",
         "-Wno-format-truncation",
         "-I" + os.path.join(H.ROOT, "include"), "-I" + csrc,
         os.path.join(H.ROOT, "scripts", "extend_edist_host_check.c"),
         os.path.join(csrc, "extend_edist_host.c"),
         os.path.join(csrc, "match_sink.c"), "-o", exe, "-lm", "-lpthread"])

    def run(sc, seeds, L, K, S, threads):
        q = sc.queries()
        path = str(tmp_path / "seeds.txt")
        with open(path, "w") as f:
            sym = q.symbols if q is not None else np.zeros(0, np.uint8)
            nq = q.nq if q is not None else 0
            f.write("%d %d %d %d %d %d %d %d\n" % (
                len(sc.text), len(sym), nq, len(seeds), L, K, S, threads))
            f.write(" ".join(str(int(c)) for c in sc.text) + "\n")
            f.write(" ".join(str(int(c)) for c in sym) + "\n")
            for i in range(nq):
                f.write("%d %d\n" % (q.start[i], q.length[i]))
            for x in seeds:
                f.write("%d %d %d %d\n" % tuple(int(v) for v in x))
        return subprocess.run([exe, path], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE)

    for name in DC.SCENARIOS:
        sc = SC[name]
        L, K, S = sc.params[1]
        p = run(sc, sc.records(), L, K, S, 2)
        assert p.returncode == 0, p.stderr.decode()
        assert b"Sanitizer" not in p.stderr and b"runtime error" not in \
            p.stderr
        want = sc.model(L, K, S)
        got = np.array([[int(v) for v in l.split()]
                        for l in p.stdout.decode().splitlines()],
                       np.int64).reshape(-1, 6)
        assert np.array_equal(got[:, 0], DM.lengths1(want).astype(np.int64))
        assert np.array_equal(got[:, 1], DM.lengths2(want).astype(np.int64))
        assert np.array_equal(got[:, 2], DM.distances(want).astype(np.int64))
        for col, field in ((3, "dbstart"), (4, "queryseq"),
                           (5, "querystart")):
            assert np.array_equal(got[:, col], want[field].astype(np.int64))
    sc = SC["borders"]
    bad = sc.records()
    bad["querystart"][3] = 1 << 30
    p = run(sc, bad, 10, 2, 0, 1)
    assert p.returncode == 1 and b"record 3 does not fit" in p.stderr
    assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr
