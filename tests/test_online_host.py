"""The scan without an index on the host (vmatch -online -complete):
vsa_findcompletematches_online_host against every recorded run of the real
reference (tests/golden/online_*), row for row and in order, and the lines of
the sink against the recorded md5; the exact scan against the CPU oracle; the
literal Python model (online_model.py) against the host code on hand-made
texts at 1, 3 and 16 threads; the refusals; the host code also as a program
of its own under the sanitizers.  No GPU.

The model reproduced every recorded list in full when the fixtures were
written (scripts/make_golden_online.py writes nothing otherwise)."""
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H
import online_cases as OC
import online_model as OM

THREADS = (1, 3, 16)


def host(V, text, q, r=None, **kw):
    if r is not None:
        kw = dict(mode=r["mode"], distvalue=r["K"], percent=r["percent"],
                  removeredundant=r["remred"], **kw)
    return V.findcompletematches_online_host(text, q.symbols, q.start,
                                             q.length, **kw)


@pytest.mark.parametrize("key", OC.golden_keys())
def test_host_code_equals_every_recorded_list(V, key):
    r, e = OC.run_of(key), OC.manifest()[key]
    t = OC.text_of(r)
    want = OC.expected_rows(key)
    assert len(want) == e["lines"] and (key in OC.EMPTY) == (len(want) == 0)
    rows, text = [], []
    for pal, q in OC.passes(r):
        got = host(V, t.tis, q, r, threads=3)
        rows.append(OC.rows_of(r, got, pal))
        text.append(V.Sink(**OC.sink_kwargs(V, r, pal)).format(got))
    assert np.array_equal(np.concatenate(rows), want)
    if len(want):
        assert OC.md5(b"".join(text)) == e["md5_lines"]


def test_the_recorded_runs_are_the_ones_the_issue_names():
    m = OC.manifest()
    assert set(m) == set(OC.golden_keys()) and len(m) == 40
    for key, e in m.items():
        assert e["lines"] <= 6000 and "-online" in e["args"] and \
            "-complete" in e["args"]
    assert {(e["text"], e["mode"], e["K"]) for e in m.values()
            if e["text"] == "micro" and e["strands"] == "d"} == \
        {("micro", OC.EXACT, 0), ("micro", OC.HAMMING, 1),
         ("micro", OC.HAMMING, 2), ("micro", OC.EDIST, 1),
         ("micro", OC.EDIST, 2)}
    at = {k: e for k, e in m.items() if e["text"] == "at1mb"}
    assert sorted(at) == ["at1mb_e2", "at1mb_e3_remred", "at1mb_e5p",
                          "at1mb_h10p", "at1mb_h3"]
    assert {32, 33, 64, 65, 130} <= set(at["at1mb_e2"]["lengths"])
    assert 0 in at["at1mb_e5p"]["thresholds"]
    assert any(e["strands"] == "dp" for e in m.values())
    # what the runs show between them: a hit that did not improve was
    # dropped, a maxlength cut by the end of the text, a wildcard facing a
    # wildcard under -h, a raw-equality hit beyond 64 symbols, a distance
    # above the threshold reported as it came
    assert m["tandem_e2_remred"]["dropped"] > 0
    assert m["tandem_e2_remred"]["lines"] < m["tandem_e2"]["lines"]
    assert any(e["cutbyend"] > 0 for e in m.values())
    assert any(e["wildvswild"] > 0 for e in m.values())
    assert any(e["rawhits"] > 0 for e in m.values())
    assert any(e["abovethreshold"] > 0 for e in m.values())
    # a read longer than its text; low complexity: remred drops more than
    # 1000 hits of a run of start positions as long as the text
    assert any(max(e["lengths"], default=0) > OC.text_of(OC.run_of(k)).n or
               max(OC.reads_of(OC.run_of(k)).length) >
               OC.text_of(OC.run_of(k)).n for k, e in m.items())
    assert any(e["remred"] and e["dropped"] > 1000 and
               m[k.replace("_remred", "")]["lines"] - e["lines"] > 1000
               for k, e in m.items())
    for name in ("homopolymer", "period2", "period3", "tiny7", "tiny8",
                 "tiny9"):
        assert os.path.getsize(os.path.join(
            H.GOLDEN, "online_%s.fna" % name)) < 1024
    r = OC.run_of("grumbach_exact_short")
    assert max(OC.reads_of(r).length) < OC.text_of(r).prefixlength
    for name in ("online_manifest.json", "online_expected.npz"):
        assert os.path.getsize(os.path.join(H.GOLDEN, name)) <= 64 * 1024


@pytest.mark.parametrize("case", ["micro", "grumbach", "c6"])
def test_exact_scan_equals_the_oracle(V, case):
    idx, q = H.load_case(case)
    if case == "grumbach":
        q = OC.reads_of(OC.run_of("grumbach_exact_short"))
    want = H.oracle_complete(idx, q, online=True)
    for threads in THREADS:
        got = host(V, idx.tis, q, mode=OC.EXACT, threads=threads)
        assert np.array_equal(got, want)
    assert len(want) > 0


def edges():
    out = [(OC.borders_edge(m, k), k) for m in (1, 8, 32, 33, 64, 65, 129)
           for k in OC.thresholds(m)]
    out += [(OC.remred_edge(), k) for k in (1, 2, 3)]
    out += [(OC.wildcard_edge(m, 2), 2) for m in (40, 64, 65, 70)]
    return out


def test_model_and_host_code_agree_on_hand_made_texts(V):
    dropped = compared = 0
    for edge, k in edges():
        q = edge.queries()
        for mode, remred in ((OC.EXACT, False), (OC.HAMMING, False),
                             (OC.EDIST, False), (OC.EDIST, True)):
            info = {}
            want = OM.findcompletematches(edge.text, edge.reads, mode, k,
                                          False, remred, offset=7, info=info)
            dropped += info.get("dropped", 0) if remred else 0
            for threads in THREADS:
                got = host(V, edge.text, q, mode=mode, distvalue=k,
                           removeredundant=remred, offset=7, threads=threads)
                assert np.array_equal(got, want), (edge.name, mode, remred,
                                                   threads)
            compared += len(want)
    assert dropped > 0 and compared > 1000
    # percent thresholds, one of them 0
    edge = OC.Edge("percent", OC.borders_edge(33, 1).text,
                   OC.borders_edge(33, 1).reads[:1] +
                   [OC.borders_edge(33, 1).reads[0][:12]])
    want = OM.findcompletematches(edge.text, edge.reads, OC.EDIST, 5, True)
    got = host(V, edge.text, edge.queries(), mode=OC.EDIST, distvalue=5,
               percent=True, threads=3)
    assert np.array_equal(got, want) and len(want) > 0
    assert set(want["querystart"][want["queryseq"] == 1]) == {0}


def test_host_code_takes_what_the_device_refuses_and_refuses_the_rest(V):
    edge = OC.borders_edge(8, 1)
    q = edge.queries()
    # a threshold >= m: every position of a sequence matches
    want = OM.findcompletematches(edge.text, edge.reads[:1], OC.EDIST, 8)
    got = V.findcompletematches_online_host(edge.text, edge.reads[0], [0],
                                            [8], OC.EDIST, 8, threads=3)
    assert np.array_equal(got, want)
    assert len(want) == int((edge.text != OC.SEP).sum())
    # an alphabet of 20 symbols, 600 symbols: any m, any alphabet
    rng = np.random.default_rng(3)
    text = rng.integers(0, 20, 3000).astype(np.uint8)
    read = text[1000:1600].copy()
    read[[5, 300]] = (read[[5, 300]] + 1) % 20
    for mode in (OC.EXACT, OC.HAMMING, OC.EDIST):
        want = OM.findcompletematches(text, [read], mode, 3)
        got = V.findcompletematches_online_host(text, read, [0], [600], mode,
                                                3, threads=3)
        assert np.array_equal(got, want)
    for kw, code, word in (
            (dict(mode=3), -2, "mode 3"),
            (dict(mode=-1), -2, "mode -1"),
            (dict(mode=OC.EXACT, removeredundant=True), -2,
             'argument "remred" of option -complete requires options -e or '
             '-h'),
            (dict(mode=OC.HAMMING, distvalue=1, removeredundant=True), -2,
             "remred"),
            (dict(mode=OC.EDIST, distvalue=10, percent=2), V.NOT_COVERED,
             "Kb")):
        with pytest.raises(V.VsaError) as e:
            host(V, edge.text, q, **kw)
        assert e.value.code == code and word in e.value.message
    with pytest.raises(V.VsaError) as e:
        host(V, edge.text, q, mode=OC.EDIST, distvalue=1, capacity=3)
    assert e.value.code == -3 and "more than 3 matches" in e.value.message


def test_every_entry_of_the_header_has_its_mirror(V):
    text = open(os.path.join(H.ROOT, "include", "vstree_amd_online.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(vsa_[a-z0-9_]+)\s*\(", text)))
    assert len(syms) == 8 and syms == V.ONLINE_ABI_SYMBOLS
    out = subprocess.check_output(["nm", "-D", "--defined-only",
                                   V.LIBPATH_NORT]).decode()
    have = {l.split()[-1] for l in out.splitlines() if l}
    assert set(syms) <= have
    assert re.search(r"#define VSA_ONLINE_TILE_DEFAULT\s+%du\b"
                     % V.ONLINE_TILE_DEFAULT, text)
    assert OC.H_TILE == V.ONLINE_TILE_DEFAULT
    assert re.search(r"#define VSA_ONLINE_COUNTERS_DEFAULT\s+\(1ull << 26\)",
                     text) and V.ONLINE_COUNTERS_DEFAULT == 1 << 26
    main = open(os.path.join(H.ROOT, "include", "vstree_amd.h")).read()
    assert '#include "vstree_amd_online.h"' in main


def test_host_code_under_the_sanitizers_as_a_program_of_its_own(tmp_path):
    """online_host.c with the rules and scripts/online_host_check.c built
    with -fsanitize=address,undefined: the sliced scan against the unsliced
    one and against the model, no Python and no GPU in the process"""
    exe = str(tmp_path / "online_host_check")
    csrc = os.path.join(H.ROOT, "vstree_amd", "csrc")
    subprocess.check_call(
        ["gcc", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-Wall", "-Wextra",
         "-Wno-format-truncation",
         "-I" + os.path.join(H.ROOT, "include"), "-I" + csrc,
         os.path.join(H.ROOT, "scripts", "online_host_check.c"),
         os.path.join(csrc, "online_host.c"), "-o", exe, "-lm", "-lpthread"])

    def run(edge, mode, k, remred, threads, percent=0):
        q = edge.queries()
        path = str(tmp_path / "batch.txt")
        with open(path, "w") as f:
            f.write("%d %d %d %d %d %d %d %d\n" % (
                len(edge.text), len(q.symbols), q.nq, mode, k, percent,
                int(remred), threads))
            f.write(" ".join(str(int(c)) for c in edge.text) + "\n")
            f.write(" ".join(str(int(c)) for c in q.symbols) + "\n")
            for i in range(q.nq):
                f.write("%d %d\n" % (q.start[i], q.length[i]))
        return subprocess.run([exe, path], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE)

    # (a dense text: every position a start position, runs of them as long
    # as a sequence; a tiny one: reads longer than the text, 50 percent of
    # them as the threshold)
    cases = [(OC.borders_edge(33, 3), 3, 0), (OC.borders_edge(65, 6), 6, 0),
             (OC.borders_edge(1, 0), 0, 0), (OC.remred_edge(), 2, 0),
             (OC.wildcard_edge(70, 2), 2, 0),
             (OC.dense_edge("period3sep", 2049), 3, 0),
             (OC.tiny_edge(7), 50, 1), (OC.tiny_edge(9, True), 50, 1),
             (OC.empty_edges()[0], 0, 0)]
    for edge, k, percent in cases:
        for mode, remred in ((OC.EXACT, False), (OC.HAMMING, False),
                             (OC.EDIST, False), (OC.EDIST, True)):
            p = run(edge, mode, k, remred, 5, percent)
            assert p.returncode == 0, p.stderr.decode()
            assert b"Sanitizer" not in p.stderr and b"runtime error" not in \
                p.stderr
            want = OC.model(edge, mode, k, bool(percent), remred) \
                if hasattr(edge, "Ks") else \
                OM.findcompletematches(edge.text, edge.reads, mode, k,
                                       False, remred)
            got = np.array([[int(v) for v in l.split()]
                            for l in p.stdout.decode().splitlines()],
                           np.int64).reshape(-1, 4)
            for i, name in enumerate(("length", "dbstart", "queryseq",
                                      "querystart")):
                assert np.array_equal(got[:, i], want[name].astype(np.int64))
    p = run(cases[0][0], 5, 1, False, 2)
    assert p.returncode == 1 and b"mode 5" in p.stderr
    assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr
