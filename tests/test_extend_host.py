"""The Hamming extension of exact seeds on the host (vmatch -l L -h K outside
-complete): the pure-Python model (extend_model.py) and
vsa_extend_hamming_host, fed with the seed lists of the CPU oracle, against
every recorded run of the real reference (tests/golden/extend_*), row for row
and in order; the lines of the sink against the recorded md5; the reference's
error; the hand-made border cases, model against host code, the host code
also as a program of its own under the sanitizers.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import extend_cases as EC
import extend_model as EM
import helpers as H


_seeds = {}


def seeds_of(key):
    """[(palindromic, batch or None, seed list of the oracle)] of a run"""
    if key not in _seeds:
        r = EC.run_of(key)
        _seeds[key] = [(pal, q, EC.oracle_seeds(r, q))
                       for pal, q in EC.passes(r)]
    return _seeds[key]


def triple(q):
    return None if q is None else (q.symbols, q.start, q.length)


@pytest.mark.parametrize("key", EC.golden_keys())
def test_model_and_host_code_equal_every_recorded_list(V, key):
    r, e = EC.run_of(key), EC.manifest()[key]
    idx, _ = EC.load(r)
    want = EC.expected_rows(key)
    assert len(want) == e["lines"]
    model, host, text = [], [], []
    for pal, q, seeds in seeds_of(key):
        rec = EM.extend(seeds, idx.tis, idx.numofchars, r["L"], r["K"],
                        r["S"], triple(q))
        got = V.extend_hamming_host(idx.tis, seeds, r["L"], r["K"], r["S"],
                                    queries=triple(q),
                                    numofchars=idx.numofchars, threads=3)
        assert np.array_equal(got, rec)
        model.append(EC.rows_of(r, rec, pal))
        host.append(EC.rows_of(r, got, pal))
        text.append(V.Sink(**EC.sink_kwargs(V, r, pal)).format(got))
    assert np.array_equal(np.concatenate(model), want)
    assert np.array_equal(np.concatenate(host), want)
    assert int(want[:, 5].max()) == e["maxdistance"] <= r["K"]
    assert EC.md5(b"".join(text)) == e["md5_lines"]


def test_the_recorded_runs_are_the_ones_the_issue_names():
    m = EC.manifest()
    assert set(m) == {r["key"] for r in EC.RUNS}
    for key in EC.golden_keys():
        assert 0 < m[key]["lines"] <= 6000
    # extensions of thousands of symbols, and distances up to the bound
    assert m["ychr3_l200_h20"]["maxlength"] > 2000
    assert m["at1mb_l100_h8"]["maxdistance"] == 8
    assert m["micro_q_l8_h1"]["maxdistance"] == 1
    for name in ("extend_manifest.json", "extend_expected.npz"):
        assert os.path.getsize(os.path.join(H.GOLDEN, name)) <= 300 * 1024


def test_seed_length_rule_and_the_recorded_error(V):
    for L, K, S in ((40, 2, 0), (40, 2, 20), (10, 2, 0), (100, 8, 0),
                    (7, 7, 0), (3, 5, 2)):
        assert V.extend_seedlength(L, K, S) == EM.seedlength_rule(L, K, S) \
            == max(S, L // (K + 1))
    # L / (K + 1) below the prefix length: what the reference says, which is
    # what the engine's search says for that seed length
    r = EC.run_of("c5_q_l10_h2")
    idx, q = EC.load(r)
    text = EC.manifest()[r["key"]]["stderr"]
    assert text == "searchlength=%d must be >= %d=prefixlen" % (
        EC.seedlength(r), idx.prefixlength)
    with pytest.raises(H.OracleError) as e:
        EC.oracle_seeds(r, q)
    assert str(e.value) == text


SC = EC.scenarios(256, 1024)


def test_the_limits_the_scenarios_are_built_around(V):
    assert (V.EXTEND_LANE_BUDGET, V.EXTEND_LONG_STEP) == (256, 1024)
    assert V.EXTEND_LANE_BUDGET % 8 == 0 and V.EXTEND_LONG_STEP == 64 * 16
    assert V.EXTEND_MAXDIST >= 32
    assert len(EC.alignment_residues(SC["alignment"])) == 64
    for sc in SC.values():
        assert len(sc.text) <= 8192 and len(sc.seeds) <= 2048


@pytest.mark.parametrize("name", EC.SCENARIOS)
def test_host_code_equals_the_model_on_the_border_cases(V, name):
    sc = SC[name]
    q, seeds = sc.queries(), sc.records()
    some = 0
    for L, K, S in sc.params + [(30, 200, 0)]:
        want = sc.model(L, K, S)
        for threads in (1, 4):
            got = V.extend_hamming_host(sc.text, seeds, L, K, S,
                                        queries=triple(q), threads=threads)
            assert np.array_equal(got, want), (L, K, S)
        some += len(want)
    assert some > 0
    # a list in which every seed is dropped, and an empty list
    assert len(V.extend_hamming_host(sc.text, seeds, 100000, 2,
                                     queries=triple(q))) == 0
    assert len(V.extend_hamming_host(sc.text, seeds[:0], 20, 2,
                                     queries=triple(q))) == 0


def test_host_code_refuses_what_does_not_fit(V):
    sc = SC["borders"]
    q, seeds = sc.queries(), sc.records()
    for field, value in (("dbstart", len(sc.text)), ("queryseq", q.nq),
                         ("querystart", 1 << 20), ("length", 0),
                         ("length", 1 << 50)):
        bad = seeds.copy()
        bad[field][5] = value
        with pytest.raises(V.VsaError) as e:
            V.extend_hamming_host(sc.text, bad, 10, 2, queries=triple(q))
        assert e.value.code == -2 and "record 5 does not fit" in \
            e.value.message
    for L, K in ((0, 2), (10, 0), (10, 1 << 16)):
        with pytest.raises(V.VsaError) as e:
            V.extend_hamming_host(sc.text, seeds, L, K, queries=triple(q))
        assert e.value.code == -2


def test_every_extend_entry_of_the_header_has_its_mirror(V):
    text = open(os.path.join(H.ROOT, "include", "vstree_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = set(re.findall(r"\b(vsa_(?:extend|find[a-z]+_hamming)[a-z0-9_]*)"
                          r"\s*\(", text))
    assert len(syms) == 8 and syms <= set(V.ABI_SYMBOLS)
    assert (V.SINK_QUERY_HAMMING, V.SINK_SELF_HAMMING) == (8, 9)
    assert V.HAMMING_LENGTHBITS == EM.LENGTHBITS == 48


def test_handles_refuse_layouts_of_extended_seeds(V):
    lay = V.sink_params(kind=V.SINK_SELF_HAMMING, totallength=1000,
                        markpos=[])
    rec = np.zeros(2, V.MATCH_DTYPE)
    rec["length"] = 20
    for call in (lambda: V.select_host(lay, rec),
                 lambda: V.chain_host(lay, rec)):
        with pytest.raises(V.VsaError) as e:
            call()
        assert e.value.code == V.NOT_COVERED
        assert "extended seeds" in e.value.message


def test_host_code_under_the_sanitizers_as_a_program_of_its_own(tmp_path):
    """extend_host.c with the rules, match_sink.c (the E-value table) and
    scripts/extend_host_check.c built with -fsanitize=address,undefined: the
    border cases, no Python and no GPU in the process"""
    exe = str(tmp_path / "extend_host_check")
    csrc = os.path.join(H.ROOT, "vstree_amd", "csrc")
    subprocess.check_call(
        ["gcc", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-Wall", "-Wextra",
         "-Wno-format-truncation",
         "-I" + os.path.join(H.ROOT, "include"), "-I" + csrc,
         os.path.join(H.ROOT, "scripts", "extend_host_check.c"),
         os.path.join(csrc, "extend_host.c"),
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

    for name in EC.SCENARIOS:
        sc = SC[name]
        L, K, S = sc.params[0]
        p = run(sc, sc.records(), L, K, S, 2)
        assert p.returncode == 0, p.stderr.decode()
        assert b"Sanitizer" not in p.stderr and b"runtime error" not in \
            p.stderr
        want = sc.model(L, K, S)
        got = np.array([[int(v) for v in l.split()]
                        for l in p.stdout.decode().splitlines()],
                       np.int64).reshape(-1, 5)
        assert np.array_equal(got[:, 0], EM.lengths(want).astype(np.int64))
        assert np.array_equal(got[:, 1], EM.distances(want).astype(np.int64))
        for col, field in ((2, "dbstart"), (3, "queryseq"),
                           (4, "querystart")):
            assert np.array_equal(got[:, col], want[field].astype(np.int64))
    sc = SC["borders"]
    bad = sc.records()
    bad["querystart"][3] = 1 << 30
    p = run(sc, bad, 10, 2, 0, 1)
    assert p.returncode == 1 and b"record 3 does not fit" in p.stderr
    assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr
