"""vmatch -s on the host (no GPU): vsa_align_host against the scripts the
literal Python model (align_model.py) made for every recorded run of the real
reference -- the generator trusted them because the text they print IS the
reference's --, vsa_align_format against the recorded text and md5 of every
run, both against the model on the match lists made by hand, and what the two
entries refuse."""
import os
import re

import numpy as np
import pytest

import align_cases as AC
import align_model as AM
import helpers as H

KEYS = [r["key"] for r in AC.RUNS]


def run_passes(V, key):
    """-> [(palindromic, records, offsets, words)] from vsa_align_host"""
    r = AC.run_of(key)
    db, q = AC.load(r["case"])
    qt = (q.symbols, q.start, q.length) if r["q"] else None
    out = []
    for pal, rows in AC.passes(r, AC.expected(key, "rows")):
        rec = AC.records_of(r, rows)
        offsets, words = V.align_host(r["kind"], db.symbols, rec, qt, pal)
        out.append((pal, rec, offsets, words))
    return out


def format_pass(V, r, pal, rec, offsets, words, **more):
    db, q = AC.load(r["case"])
    sink = V.Sink(**AC.sink_kwargs(V, r, pal, **more))
    qt = (q.symbols, q.start, q.length) if r["q"] else None
    return V.align_format(sink, rec, offsets, words, db.symbols, db.orig, qt,
                          q.orig if r["q"] else None, r["width"])


def joined(parts):
    """the passes of a run as one CSR"""
    offsets, base = [np.zeros(1, np.uint64)], 0
    for _, _, o, w in parts:
        offsets.append(o[1:] + np.uint64(base))
        base += len(w)
    return np.concatenate(offsets), np.concatenate([w for *_, w in parts])


@pytest.mark.parametrize("key", KEYS)
def test_host_scripts_are_the_models_on_every_recorded_run(V, key):
    offsets, words = joined(run_passes(V, key))
    assert np.array_equal(offsets, AC.expected(key, "offsets"))
    assert np.array_equal(words, AC.expected(key, "words"))
    assert len(words) == AC.manifest()[key]["words"]


@pytest.mark.parametrize("key", KEYS)
def test_formatted_text_has_the_recorded_md5(V, key):
    r, e = AC.run_of(key), AC.manifest()[key]
    text = b"".join(format_pass(V, r, *part) for part in run_passes(V, key))
    assert len(text) == e["bytes"]
    assert AC.md5(text) == e["md5"]
    first = "".join(e["first"]).encode()
    assert text[:len(first)] == first
    # several formatting threads, the same text in the same order
    if e["matches"] > 2000:
        again = b"".join(format_pass(V, r, *part, threads=5)
                         for part in run_passes(V, key))
        assert again == text


def test_recorded_runs_hold_every_class_of_alignment():
    import json
    with open(os.path.join(H.GOLDEN, "align_manifest.json")) as f:
        classes = json.load(f)["classes"]
    assert all(classes[k] > 0 for k in ("indel", "palindromic", "sametext",
                                        "overshoot", "wildcard"))
    for name in ("align_manifest.json", "align_expected.npz"):
        assert os.path.getsize(os.path.join(H.GOLDEN, name)) <= 400000
    kinds = {e["kind"] for e in AC.manifest().values()}
    assert kinds == {0, 1, 2, 3, 4, 8, 9, 10, 11}


# --------------------------------------------------------------------------
# match lists made by hand
# --------------------------------------------------------------------------

def scenarios():
    out = [AC.planted_distance(D) for D in AC.DISTANCES]
    out += [AC.planted_distance(8, True), AC.planted_tandem(),
            AC.planted_tandem(AC.QUERY_EDIST), AC.planted_overshoot(),
            AC.planted_mixed(AC.QUERY_HAMMING), AC.planted_mixed(AC.QUERY),
            AC.planted_mixed(AC.QUERY_EDIST, 64)]
    return {sc.name: sc for sc in out}


SCENARIOS = scenarios()


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_hand_made_lists_equal_the_model(V, name):
    sc = SCENARIOS[name]
    rec = sc.records()
    want = sc.model()
    for threads in (1, 3):
        got = V.align_host(sc.kind, sc.text, rec, sc.triple(), sc.palindromic,
                           threads)
        assert np.array_equal(got[0], want[0])
        assert np.array_equal(got[1], want[1])
    # ... and the text of the model's own formatter
    q = sc.queries()
    kw = dict(kind=sc.kind, totallength=len(sc.text), markpos=[],
              palindromic=sc.palindromic)
    if q is not None:
        kw.update(querystart=q.start, querylength=q.length,
                  querytotallength=len(q.symbols))
    sink = V.Sink(**kw)
    text = V.align_format(sink, rec, want[0], want[1], sc.text,
                          AC.LETTERS[sc.text], sc.triple(),
                          None if q is None else AC.LETTERS[q.symbols], 37)
    lines = sink.format(rec).split(b"\n")[:-1]
    model = b""
    for i, (x, pair) in enumerate(zip(rec, sc.pairs())):
        words = [int(w) for w in want[1][int(want[0][i]):int(want[0][i + 1])]]
        assert AM.consumed(words) == (len(pair.u), len(pair.v))
        model += lines[i] + b"\n" + pair.show(words, 37)
    assert text == model


def test_scenarios_cover_what_they_are_meant_to(V):
    assert V.ALIGN_MAXDIST == 31 == max(AC.DISTANCES)
    for D in AC.DISTANCES:
        sc = SCENARIOS["distance%d" % D]
        pairs = sc.pairs()
        real = [AM.fronts(p.u, p.v, p.distance).distance for p in pairs]
        assert all(p.distance == D for p in pairs) and max(real) == D
        # the end diagonal on the outermost lane, either side
        assert {len(p.v) - len(p.u) for p in pairs} >= {-D, D}
        if D > 1:
            assert min(real) < D                  # stored above the real one
            assert any((p.u >= AC.WILD).any() for p in pairs)
            assert any((p.v >= AC.WILD).any() for p in pairs)
        starts = {int(x) for x in sc.records()["dbstart"]}
        assert 0 in starts and any(
            int(x["dbstart"]) + len(p.u) == len(sc.text)
            for x, p in zip(sc.records(), pairs))
        words = [p.script() for p in pairs]
        assert any(w[-1] in (AM.INSERTIONEOP, AM.DELETIONEOP) for w in words)
        assert D == 1 or any(w[0] in (AM.INSERTIONEOP, AM.DELETIONEOP)
                             for w in words)
    # the shortcut: a diagonal within the distance is the same text
    reached = 0
    for p in SCENARIOS["tandem"].pairs():
        f = AM.fronts(p.u, p.v, p.distance, p.sametext)
        reached += 0 < abs(p.sametext) <= f.distance
    assert reached >= 4
    with_shortcut = SCENARIOS["tandem"].model()
    without = SCENARIOS["tandem_as_queries"].model()
    assert not (np.array_equal(with_shortcut[0], without[0]) and
                np.array_equal(with_shortcut[1], without[1]))
    # the backward slide passes the start of the forward one
    for p in SCENARIOS["overshoot"].pairs():
        f = AM.fronts(p.u, p.v, p.distance)
        assert AM.backtrace(f, p.u, p.v)[1]
    rec = SCENARIOS["mixed8_65"].records()
    d = V.hamming_distances(rec)
    assert (d == 0).any() and (d > 0).any() and len(rec) == 65


def test_a_run_of_more_than_16383_symbols_is_cut_like_the_reference(V):
    sc = AC.planted_longrun()
    want = sc.model()
    got = V.align_host(sc.kind, sc.text, sc.records())
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # ADDIDENTICAL's pieces, literally: lenid & 16383 first
    assert list(got[1][:3]) == [1999, 0xC000, 18000 & 16383]
    assert got[1][3] == (18000 - 16383) and got[0][1] == 4
    # ... which do not add up: such a script is not printed
    sink = V.Sink(kind=sc.kind, totallength=len(sc.text), markpos=[])
    with pytest.raises(V.VsaError) as e:
        V.align_format(sink, sc.records(), got[0], got[1], sc.text,
                       AC.LETTERS[sc.text])
    assert e.value.code == -2 and "does not account" in e.value.message


def test_what_the_host_entries_refuse(V):
    sc = SCENARIOS["distance7"]
    rec, qt = sc.records(), sc.triple()
    ok = V.align_host(sc.kind, sc.text, rec, qt)
    assert len(ok[0]) == len(rec) + 1
    # kinds without an alignment here
    for kind in (5, 6, 12, 13, 14, 15, 7, 16):
        with pytest.raises(V.VsaError) as e:
            V.align_host(kind, sc.text, rec, qt)
        assert e.value.code == V.NOT_COVERED
    # a self kind takes no batch and no -p pass; a query kind needs its batch
    for call in (lambda: V.align_host(AC.SELF_EDIST, sc.text, rec, None, True),
                 lambda: V.align_host(sc.kind, sc.text, rec, None)):
        with pytest.raises(V.VsaError) as e:
            call()
        assert e.value.code == -2
    # records that do not fit their texts, or that no matcher delivers
    n = len(sc.text)
    for field, value in (("dbstart", n - 3), ("queryseq", len(sc.reads)),
                         ("querystart", 1 << 33), ("length", 0),
                         ("length", 5 | 7 << 48),          # distance > length
                         ("length", 90 | 2 << 48 | 9 << 56)):   # 9 > distance
        bad = rec.copy()
        bad[field][2] = value
        with pytest.raises(V.VsaError) as e:
            V.align_host(sc.kind, sc.text, bad, qt)
        assert e.value.code == -2
        assert "record 2 does not fit" in e.value.message
    # a distance below the real one is the reference's error
    low = rec.copy()
    low["length"][0] = (int(low["length"][0]) & ~(0xFF << 48)) | 3 << 48
    with pytest.raises(V.VsaError) as e:
        V.align_host(sc.kind, sc.text, low, qt)
    assert e.value.code == -2 and "record 0" in e.value.message
    # the words do not fit: the offsets say how many there are
    offsets = np.zeros(len(rec) + 1, np.uint64)
    words = np.zeros(3, np.uint16)
    p, keep = V.sink_params(sc.kind, len(sc.text), (), querystart=qt[1],
                            querylength=qt[2])
    rc = V.lib.vsa_align_host(V.C.byref(p), V._ptr(sc.text), V._ptr(qt[0]),
                              V._ptr(rec), len(rec), 0, 1, V._ptr(offsets),
                              V._ptr(words), 3)
    assert rc == -3 and np.array_equal(offsets, ok[0]) and not words.any()
    # an empty list
    empty = V.align_host(sc.kind, sc.text, rec[:0], qt)
    assert list(empty[0]) == [0] and len(empty[1]) == 0
    # the formatter wants the scripts of its records
    sink = V.Sink(kind=sc.kind, totallength=n, markpos=[], querystart=qt[1],
                  querylength=qt[2], querytotallength=len(qt[0]))
    with pytest.raises(V.VsaError) as e:
        V.align_format(sink, rec, ok[0], ok[1][::-1].copy(), sc.text,
                       AC.LETTERS[sc.text], qt, AC.LETTERS[qt[0]])
    assert e.value.code == -2
    small = np.zeros(10, np.uint8)
    n = V.lib.vsa_align_format(sink._h, V._ptr(rec), len(rec), V._ptr(ok[0]),
                               V._ptr(ok[1]), V._ptr(sc.text),
                               V._ptr(AC.LETTERS[sc.text]), V._ptr(qt[0]),
                               V._ptr(AC.LETTERS[qt[0]]), 0, V._ptr(small), 10)
    assert n == -3


def test_write_prints_what_format_returns(V, tmp_path):
    key = "micro_q_l8_e1_s30"
    r = AC.run_of(key)
    db, q = AC.load(r["case"])
    (pal, rec, offsets, words), = run_passes(V, key)
    sink = V.Sink(**AC.sink_kwargs(V, r, pal))
    libc = V.C.CDLL(None)
    libc.fopen.restype = V.C.c_void_p
    libc.fclose.argtypes = [V.C.c_void_p]
    path = str(tmp_path / "out.txt")
    f = libc.fopen(path.encode(), b"w")
    assert f
    rc = V.lib.vsa_align_write(sink._h, V._ptr(rec), len(rec), V._ptr(offsets),
                               V._ptr(words), V._ptr(db.symbols),
                               V._ptr(db.orig), V._ptr(q.symbols),
                               V._ptr(q.orig), r["width"], f)
    libc.fclose(f)
    assert rc == 0
    with open(path, "rb") as g:
        assert AC.md5(g.read()) == AC.manifest()[key]["md5"]


def test_binding_and_header_name_the_same_entries(V):
    text = open(os.path.join(H.ROOT, "include", "vstree_amd_align.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(vsa_[a-z0-9_]+)\s*\(", text)))
    assert len(syms) == 8 and syms == V.ALIGN_ABI_SYMBOLS


def test_host_code_under_the_sanitizers_as_a_program_of_its_own(V, tmp_path):
    """align_host.c with the rules, match_sink.c (the match lines) and
    scripts/align_host_check.c built with -fsanitize=address,undefined: the
    match lists made by hand through vsa_align_host and vsa_align_format in
    arrays of exactly their sizes, no Python and no GPU in the process"""
    import subprocess
    exe = str(tmp_path / "align_host_check")
    csrc = os.path.join(H.ROOT, "vstree_amd", "csrc")
    subprocess.check_call(
        ["gcc", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-Wall", "-Wextra",
         "-Wno-format-truncation",
         "-I" + os.path.join(H.ROOT, "include"), "-I" + csrc,
         os.path.join(H.ROOT, "scripts", "align_host_check.c"),
         os.path.join(csrc, "align_host.c"),
         os.path.join(csrc, "match_sink.c"), "-o", exe, "-lm", "-lpthread"])
    for name in ("distance1", "distance16", "distance31", "distance8p",
                 "tandem", "tandem_as_queries", "overshoot", "mixed8_65",
                 "mixed1_65", "mixed10_64"):
        sc = SCENARIOS[name]
        rec, q = sc.records(), sc.queries()
        sym = q.symbols if q is not None else np.zeros(0, np.uint8)
        nq = q.nq if q is not None else 0
        width, threads = (23, 1) if name == "distance16" else (0, 2)
        path = str(tmp_path / "list.txt")
        with open(path, "w") as f:
            f.write("%d %d %d %d %d %d %d %d\n" % (
                sc.kind, sc.palindromic, len(sc.text), len(sym), nq, len(rec),
                width, threads))
            f.write(" ".join(str(int(c)) for c in sc.text) + "\n")
            f.write(" ".join(str(int(c)) for c in sym) + "\n")
            for i in range(nq):
                f.write("%d %d\n" % (q.start[i], q.length[i]))
            for x in rec:
                f.write("%d %d %d %d\n" % tuple(int(v) for v in x))
        p = subprocess.run([exe, path], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE)
        assert p.returncode == 0, (name, p.stderr.decode()[-2000:])
        first, second, text = p.stdout.split(b"\n", 2)
        want = sc.model()
        assert [int(x) for x in first.split()] == [int(x) for x in want[0]]
        assert [int(x) for x in second.split()] == [int(x) for x in want[1]]
        kw = dict(kind=sc.kind, totallength=len(sc.text), markpos=[],
                  palindromic=sc.palindromic)
        if q is not None:
            kw.update(querystart=q.start, querylength=q.length,
                      querytotallength=len(q.symbols))
        assert text == V.align_format(
            V.Sink(**kw), rec, want[0], want[1], sc.text, AC.LETTERS[sc.text],
            sc.triple(), None if q is None else AC.LETTERS[q.symbols], width)
