"""Match clustering without a GPU: vsa_matchcluster_host and both replays of
the pure-Python model (matchcluster_model.py) against the recorded runs of
the real reference (members, edges in file order, values, the md5 of the
printed text and of every cluster file), against each other on random lists
full of ties and piles, and -- where the reference programs are built -- the
recorded runs once more against the live reference."""
import gzip
import os
import re
import shutil

import numpy as np
import pytest

import helpers as H
import cluster_model as CM
import matchcluster_cases as MC
import matchcluster_model as MM
import vstree_amd as V


def host_as_model(layout, rec, mode, value):
    got = V.matchcluster_host(layout, mode, value, rec)
    got["stats"] = got["stats"].asdict()
    return got


def same(got, want):
    gs, ws = dict(got["stats"]), dict(want["stats"])
    gs.pop("rounds"), ws.pop("rounds")
    assert gs == ws
    for k in ("clusterstart", "members", "labels", "edgestart", "m0", "m1",
              "values"):
        assert np.array_equal(got[k], want[k]), k
    assert got["text"] == want["text"]


@pytest.mark.parametrize("key", MC.keys())
def test_recorded_runs(key):
    r = MC.run_of(key)
    rec, flags = MC.input_of(key)
    layout = V.sink_params(**MC.layout_kwargs(r))
    lines = MC.lines_of(V, r, rec, flags)
    host = V.matchcluster_host(layout, r["mode"], r["value"], rec,
                               palindromic=flags if flags.any() else None)
    host["stats"] = host["stats"].asdict()
    MC.check_against_manifest(key, host, MC.text_of(r, host, lines, flags))
    if not flags.any():
        # one pass: the library's own formatter prints the same files
        sink = MC.sink_of(V, r, palindromic=False)

        def host_text(c):
            a, b = (int(x) for x in host["clusterstart"][c:c + 2])
            e0, e1 = (int(x) for x in host["edgestart"][c:c + 2])
            mem = host["members"][a:b]
            return V.matchcluster_format_host(
                sink, r["mode"], mem, rec[mem.astype(np.int64)],
                host["m0"][e0:e1], host["m1"][e0:e1], host["values"][e0:e1])
        MC.check_against_manifest(key, host, host_text)
    for replay in (CM.full_replay, CM.forest_replay):
        want = MC.model_of(r, rec, flags, replay=replay)
        same(host, want)
        MC.check_against_manifest(key, want,
                                  MC.text_of(r, want, lines, flags))


def random_list(rng):
    n = int(rng.integers(50, 401))
    places = rng.integers(0, 50000, int(rng.integers(20, 2001)))
    rec = MC.records(rng.integers(1, 120, n), rng.choice(places, n),
                     rng.choice(places, n))
    return rec


def test_random_lists_agree_with_the_model():
    rng = np.random.default_rng(20261018)
    layout = MC.synthetic_layout(V)
    edges = 0
    for k in range(200):
        rec = random_list(rng)
        mode = k % 2
        value = int(rng.choice([0, 1, 7, 40, 300])) if mode == MM.GAP \
            else int(rng.choice([0, 1, 33, 50, 100]))
        got = host_as_model(layout, rec, mode, value)
        same(got, MC.model(rec, mode, value))
        same(got, MC.model(rec, mode, value, replay=CM.forest_replay))
        edges += got["stats"]["edges"]
    assert edges > 10000


def test_refusals_and_small_lists():
    layout = MC.synthetic_layout(V)
    rec = MC.records([10, 10], [0, 100], [50, 150])
    for mode, value in ((MM.GAP, 5), (MM.OVERLAP, 5)):
        for k in (0, 1, 2):
            got = host_as_model(layout, rec[:k], mode, value)
            assert got["stats"]["edges"] == 0 and \
                got["stats"]["clusters"] == 0
            assert got["text"] == b"# cluster %d matches\n" % k
    with pytest.raises(V.VsaError) as e:
        V.matchcluster_host(layout, V.MATCHCLUSTER_ERATE, 5, rec)
    assert e.value.code == -4
    pal = V.sink_params(kind=1, totallength=1 << 20,
                        markpos=np.zeros(0, np.uint64), selfpalindromic=True,
                        palindromic=True)
    with pytest.raises(V.VsaError) as e:
        V.matchcluster_host(pal, MM.GAP, 5, rec)
    assert e.value.code == -4
    with pytest.raises(V.VsaError) as e:
        V.matchcluster_host(layout, MM.GAP, 5, rec, palindromic=[0, 1])
    assert e.value.code == -4


def test_a_list_against_queries_mixes_both_axes():
    # two queries of 40 symbols; the second reference is a query coordinate,
    # counted from the other end for a palindromic record
    qstart, qlen = np.array([0, 41], np.uint64), np.array([40, 40], np.uint64)
    layout = V.sink_params(kind=1, totallength=1000,
                           markpos=np.zeros(0, np.uint64), querystart=qstart,
                           querylength=qlen, querytotallength=81)
    rec = np.zeros(4, H.MATCH_DTYPE)
    rec["length"] = [10, 10, 8, 12]
    rec["dbstart"] = [5, 60, 20, 52]
    rec["queryseq"] = [0, 1, 1, 0]
    rec["querystart"] = [3, 0, 30, 20]
    flags = np.array([0, 0, 1, 1], np.uint8)
    l1, p1, p2 = MM.view(1, rec, flags, qstart, qlen)
    assert p2 == [3, 41, 43, 8]
    for mode, value in ((MM.GAP, 12), (MM.OVERLAP, 10)):
        got = V.matchcluster_host(layout, mode, value, rec, palindromic=flags)
        got["stats"] = got["stats"].asdict()
        want = MM.cluster(l1, p1, p2, mode, value)
        assert want["stats"]["edges"] > 0
        same(got, want)


def test_the_sink_prints_with_the_default_widths():
    sink = V.Sink(kind=2, totallength=1000, markpos=np.zeros(0, np.uint64))
    rec = MC.records([12], [3], [40])
    narrow = sink.format(rec)
    sink.setdigits()
    wide = sink.format(rec)
    assert narrow.split() == wide.split()
    assert wide.startswith(b"   12      0      3   D    12      0     40 ")
    with pytest.raises(V.VsaError):
        sink.setdigits(length=0)


def test_abi_names():
    syms = {s for s in V.ABI_SYMBOLS if s.startswith("vsa_matchcluster_")}
    assert len(syms) == 14 and "vsa_sink_setdigits" in V.ABI_SYMBOLS


@pytest.mark.skipif(not H.have_ref(), reason="the reference programs are "
                    "not built (make -f oracle/Makefile.ref)")
def test_recorded_runs_against_the_live_reference(tmp_path):
    wd = str(tmp_path)
    with gzip.open(os.path.join(H.GOLDEN, "at1MB.gz"), "rb") as f, \
            open(wd + "/at1MB", "wb") as g:
        g.write(f.read())
    for name in ("micro_db.fna", "micro_q.fna"):
        shutil.copy(os.path.join(H.GOLDEN, name), wd)
    for db in ("at1MB", "micro_db.fna"):
        H.run_mkvtree_ref(["-indexname", db + ".idx", "-db", db, "-pl",
                           "-dna", "-bwt", "-lcp", "-suf", "-ois", "-tis",
                           "-bck", "-sti1"], wd)
    for r in MC.RUNS:
        e = MC.manifest()[r["key"]]
        prefix = os.path.join(wd, r["key"])
        p = H.subprocess.run([H.VMATCH_REF] + MC.list_args(r) +
                             MC.cluster_args(r, prefix) +
                             [r["db"].replace(".gz", "") + ".idx"], cwd=wd,
                             stdout=H.subprocess.PIPE,
                             stderr=H.subprocess.PIPE)
        assert p.returncode == 0, p.stderr
        text = p.stdout.partition(b"\n")[2]
        assert MC.md5(text) == e["md5_text"]
        sizes = [int(x) for x in
                 re.findall(rb"of size (\d+)", text)]
        assert len(sizes) == len(e["md5_files"])
        for c, size in enumerate(sizes):
            with open("%s.%d.%d.match" % (prefix, size, c), "rb") as f:
                body = f.read().partition(b"\n")[2]
            assert MC.md5(body) == e["md5_files"][c], (r["key"], c)
