"""The scan without an index on the device (vmatch -online -complete):
vsa_findcompletematches_online on a full index and
vsa_text_findcompletematches_online on a vsa_text of the same text against
every recorded run of the real reference, rows and md5 of the sink's lines;
hand-made texts of 2000 to 5000 symbols against the literal model with tiles
of 64, 256 and the default number of symbols -- occurrences across tile
borders, at position 0 and at the end of the text, sequences shorter than
the read, separators on a tile border and m + k behind one, runs of start
positions across tile borders and with the hit remred drops --, lengths
around the word boundaries with thresholds 0, 1, 3 and m / 10, wildcards on
both sides of 64 symbols, all four forms of a batch with sequence offsets,
an online list through vsa_align and coverage, the online lists as sets
against the indexed search where the model says the sets agree, and the
refusals.  (The kernels keep text positions in 64 bits: there is no second
instantiation that VSA_FORCE_WIDE would reach; an index with 64-bit tables
is scanned once all the same.)"""
import gc

import numpy as np
import pytest

import batch_forms as BF
import helpers as H
import online_cases as OC
import online_model as OM

pytestmark = pytest.mark.gpu

TILES = (64, 256, None)
MODES = ((OC.EXACT, False), (OC.HAMMING, False), (OC.EDIST, False),
         (OC.EDIST, True))

_index, _text = {}, {}


def index_of(V, name, tis, ssp=None, host=None, wide=False):
    if (name, wide) not in _index:
        i = host if host is not None else H.oracle_build_index(tis, 4,
                                                               ssp=ssp)
        if wide:
            i = i.as_width(64)
        _index[name, wide] = V.Index.from_tables(
            i.n, i.prefixlength, i.numofchars, i.tis, i.suf, i.lcp, i.llv,
            i.bck, i.bwt, i.querysepposition, i.hasqueries)
    return _index[name, wide]


def text_of(V, name, tis, numofchars=4):
    if name not in _text:
        _text[name] = V.Text.from_host(tis, numofchars)
    return _text[name]


def settile(monkeypatch, tile):
    if tile is None:
        monkeypatch.delenv("VSA_ONLINE_TILE", raising=False)
    else:
        monkeypatch.setenv("VSA_ONLINE_TILE", str(tile))


def scan(V, where, gq, mode, k, percent=False, remred=False):
    return V.findcompletematches_online(where, gq, mode, k, percent,
                                        remred).fetch()


@pytest.mark.parametrize("key", OC.golden_keys())
def test_both_entries_equal_every_recorded_list(V, monkeypatch, key):
    settile(monkeypatch, None)
    r, e = OC.run_of(key), OC.manifest()[key]
    t = OC.text_of(r)
    want = OC.expected_rows(key)
    host = H.load_case(r["text"])[0] if not r["text"].endswith(".fna") \
        else None
    places = (index_of(V, r["text"], t.tis, t.ssp, host),
              text_of(V, r["text"], t.tis))
    for where in places:
        rows, lines = [], []
        for pal, q in OC.passes(r):
            gq = V.Queries.from_host(q.symbols, q.start, q.length)
            if pal:
                # -p is a second call on the reverse complement made on the
                # device
                fq = OC.reads_of(r)
                gq = V.Queries.from_host(fq.symbols, fq.start,
                                         fq.length).reverse_complement()
            got = scan(V, where, gq, r["mode"], r["K"], r["percent"],
                       r["remred"])
            rows.append(OC.rows_of(r, got, pal))
            lines.append(V.Sink(**OC.sink_kwargs(V, r, pal)).format(got))
        assert np.array_equal(np.concatenate(rows), want)
        if len(want):
            assert OC.md5(b"".join(lines)) == e["md5_lines"]


def check_edge(V, monkeypatch, edge, k, tiles=TILES, modes=MODES):
    q = edge.queries()
    gq = V.Queries.from_host(q.symbols, q.start, q.length)
    gt = V.Text.from_host(edge.text)
    gi = index_of(V, edge.name, edge.text)
    assert 2000 <= len(edge.text) <= 6000
    total = 0
    for mode, remred in modes:
        want = OC.model(edge, mode, k, False, remred)
        total += len(want)
        for tile in tiles:
            settile(monkeypatch, tile)
            got = scan(V, gt, gq, mode, k, False, remred)
            assert np.array_equal(got, want), (edge.name, mode, remred, tile)
        got = scan(V, gi, gq, mode, k, False, remred)
        assert np.array_equal(got, want), (edge.name, mode, remred, "index")
    return total


@pytest.mark.parametrize("m", OC.LENGTHS)
def test_tile_borders_and_word_boundaries(V, monkeypatch, m):
    for k in OC.thresholds(m):
        edge = OC.borders_edge(m, k)
        assert check_edge(V, monkeypatch, edge, k) > 0
        # what the edge was planted for: a match at position 0, one that
        # ends at n, and starts on both sides of the tile borders
        want = OC.model(edge, OC.HAMMING, k)
        starts = set(int(x) for x in want["dbstart"])
        assert 0 in starts and len(edge.text) - m in starts
        if 1 < m <= 64:
            for tile in (64, 256, OC.H_TILE):
                assert any(a // tile != (a + m - 1) // tile for a in starts)


def test_runs_of_start_positions_across_tile_borders(V, monkeypatch):
    edge = OC.remred_edge()
    for k in (1, 2, 3):
        info = {}
        OM.findcompletematches(edge.text, edge.reads, OC.EDIST, k, False,
                               True, info=info)
        assert info["dropped"] > 0
        plain = OC.model(edge, OC.EDIST, k)
        # a run of adjacent start positions that crosses a border of every
        # tile size
        pos = plain["dbstart"][plain["queryseq"] == 0].astype(np.int64)
        for tile in (64, 256, OC.H_TILE):
            assert any(a - b == 1 and a // tile != b // tile
                       for a, b in zip(pos[:-1], pos[1:]))
        check_edge(V, monkeypatch, edge, k,
                   modes=((OC.EDIST, False), (OC.EDIST, True)))


@pytest.mark.parametrize("m", (40, 64, 65, 70))
def test_wildcards_below_and_above_64_symbols(V, monkeypatch, m):
    edge = OC.wildcard_edge(m, 2)
    assert check_edge(V, monkeypatch, edge, 2) > 0
    # the wildcard of the read facing the wildcard of the text matches under
    # -h, and under -e only beyond 64 symbols
    at = OC.WILD_FACING
    h = OC.model(edge, OC.HAMMING, 0)
    assert at in set(int(x) for x in h["dbstart"][h["queryseq"] == 1])
    e = OC.model(edge, OC.EDIST, 0)
    assert (at in set(int(x) for x in e["dbstart"][e["queryseq"] == 1])) == \
        (m > 64)


@pytest.mark.parametrize("form", BF.FORMS)
def test_every_form_of_a_batch_with_offsets(V, monkeypatch, form):
    settile(monkeypatch, 64)
    edge = OC.wildcard_edge(41, 2)
    if form == "ragged":
        edge = OC.Edge(edge.name + "_ragged", edge.text,
                       edge.reads + [edge.reads[0][:17]])
    q = edge.queries()
    gt = V.Text.from_host(edge.text)
    for offset in BF.OFFSETS:
        gq = BF.device_batch(V, q, form, offset)
        for mode, remred in MODES:
            want = OC.model(edge, mode, 2, False, remred, offset=offset)
            got = scan(V, gt, gq, mode, 2, False, remred)
            assert len(want) > 0 and np.array_equal(got, want), (offset, mode)


def test_an_index_with_wide_tables_and_a_text_from_device_memory(
        V, monkeypatch):
    settile(monkeypatch, None)
    edge = OC.borders_edge(33, 3)
    q = edge.queries()
    gq = V.Queries.from_host(q.symbols, q.start, q.length)
    monkeypatch.setenv("VSA_FORCE_WIDE", "1")
    try:
        gi = index_of(V, edge.name, edge.text, wide=True)
    finally:
        monkeypatch.delenv("VSA_FORCE_WIDE")
    assert gi.info().device_integersize == 64
    d = V.device_malloc(len(edge.text))
    try:
        V.device_upload(d, edge.text)
        gt = V.Text.from_device(d, len(edge.text))
    finally:
        V.device_free(d)
    for mode, remred in MODES:
        want = OC.model(edge, mode, 3, False, remred)
        for where in (gi, gt):
            assert np.array_equal(scan(V, where, gq, mode, 3, False, remred),
                                  want)


def test_text_open_maps_the_text_alone(V, tmp_path):
    edge = OC.borders_edge(32, 1)
    name = str(tmp_path / "idx")
    with open(name + ".prj", "w") as f:
        f.write("totallength=%d\nprefixlength=3\nlargelcpvalues=0\n"
                "integersize=32\nlittleendian=1\n" % len(edge.text))
    with open(name + ".al1", "w") as f:
        f.write("aA\ncC\ngG\ntTuU\nnN\n")
    edge.text.tofile(name + ".tis")
    gt = V.Text.open(name)
    q = edge.queries()
    gq = V.Queries.from_host(q.symbols, q.start, q.length)
    assert np.array_equal(scan(V, gt, gq, OC.EDIST, 1),
                          OC.model(edge, OC.EDIST, 1))
    with pytest.raises(V.VsaError) as e:
        V.Text.open(str(tmp_path / "nothing"))
    assert "cannot open" in e.value.message


def test_an_online_list_through_align_and_coverage(V, monkeypatch):
    settile(monkeypatch, None)
    edge = OC.borders_edge(64, 3)
    q = edge.queries()
    gi = index_of(V, edge.name, edge.text)
    gq = V.Queries.from_host(q.symbols, q.start, q.length)
    for doedist, mode, kind, layout in (
            (True, OC.EDIST, V.SINK_APPROX_EDIST, V.COVERAGE_APPROX),
            (False, OC.HAMMING, V.SINK_APPROX_HAMMING, V.COVERAGE_APPROX)):
        online = V.findcompletematches_online(gi, gq, mode, 3)
        rec = online.fetch()
        indexed = V.findapproxcompletematches(gi, gq, doedist, 3).fetch()
        assert len(rec) > 0 and np.array_equal(H.sorted_matches(rec),
                                               H.sorted_matches(indexed))
        # the indexed list in the order of the online one
        key = lambda a: np.lexsort((a["dbstart"], a["queryseq"]))
        same = np.zeros(len(rec), V.MATCH_DTYPE)
        same[key(rec)] = indexed[key(indexed)]
        assert np.array_equal(same, rec)
        other = V.Result.from_host(same)
        a, b = V.align(gi, gq, online, kind), V.align(gi, gq, other, kind)
        for x, y in zip(a.fetch(), b.fetch()):
            assert np.array_equal(x, y)
        bits = []
        for res in (online, other):
            cov = V.Coverage.over_index(gi)
            cov.mark(res, layout=layout)
            bits.append(cov.bits())
            assert cov.stats().marked > 0
        assert np.array_equal(bits[0], bits[1])


def test_online_lists_as_sets_equal_the_indexed_search(V, monkeypatch):
    """where the model says the sets agree (the maxlength rule -- the end of
    the text here, the width of a region there -- can make them differ)"""
    settile(monkeypatch, None)
    compared = 0
    for m, k in ((32, 1), (33, 3), (64, 3), (65, 6), (129, 12)):
        edge = OC.borders_edge(m, k)
        q = edge.queries()
        host = H.oracle_build_index(edge.text, 4)
        gi = index_of(V, edge.name, edge.text, host=host)
        gq = V.Queries.from_host(q.symbols, q.start, q.length)
        for doedist, mode in ((True, OC.EDIST), (False, OC.HAMMING)):
            model = H.sorted_matches(OC.model(edge, mode, k))
            oracle = H.sorted_matches(H.oracle_approx(host, q, doedist, k))
            if not np.array_equal(model, oracle):
                continue
            compared += 1
            got = H.sorted_matches(scan(V, gi, gq, mode, k))
            indexed = H.sorted_matches(
                V.findapproxcompletematches(gi, gq, doedist, k).fetch())
            assert np.array_equal(got, indexed) and len(got) > 0
    assert compared >= 1


def test_refusals_deliver_nothing_and_keep_no_memory(V, monkeypatch):
    settile(monkeypatch, None)
    edge = OC.borders_edge(8, 1)
    q = edge.queries()
    gq = V.Queries.from_host(q.symbols, q.start, q.length)
    gt = V.Text.from_host(edge.text)
    gi = index_of(V, edge.name, edge.text)
    prot = V.Text.from_host(edge.text, 20)
    rng = np.random.default_rng(1)
    long = V.Queries.from_host(rng.integers(0, 4, 513).astype(np.uint8), [0],
                               [513])
    # (the wrapper asserts that no handle comes back with an error)
    scan(V, gt, gq, OC.EXACT, 0)
    gc.collect()
    free = V.device_meminfo()[0]
    for where, batch, kw, code, word in (
            (gt, gq, dict(mode=OC.EDIST, distvalue=10, percent=2),
             V.NOT_COVERED, "Kb"),
            (gi, gq, dict(mode=OC.HAMMING, distvalue=10, percent=2),
             V.NOT_COVERED, "Kb"),
            (prot, gq, dict(mode=OC.EDIST, distvalue=1), V.NOT_COVERED,
             "alphabets of 20 symbols"),
            (gt, long, dict(mode=OC.EDIST, distvalue=1), V.NOT_COVERED,
             "513 symbols"),
            (gt, gq, dict(mode=OC.EDIST, distvalue=8), V.NOT_COVERED,
             "every position matches"),
            (gt, gq, dict(mode=OC.EDIST, distvalue=100, percent=True),
             V.NOT_COVERED, "every position matches"),
            (gt, gq, dict(mode=3), -2, "mode 3"),
            (gi, gq, dict(mode=-1), -2, "mode -1"),
            (gt, gq, dict(mode=OC.EXACT, removeredundant=True), -2,
             'argument "remred" of option -complete requires options -e or '
             '-h'),
            (gi, gq, dict(mode=OC.HAMMING, distvalue=1,
                          removeredundant=True), -2, "remred")):
        with pytest.raises(V.VsaError) as e:
            V.findcompletematches_online(where, batch, **kw)
        assert e.value.code == code and word in e.value.message, kw
    # (handles of earlier tests that the collector frees in between can only
    # raise the figure; memory a refusal kept would lower it)
    assert V.device_meminfo()[0] >= free
    # modes 0 and 2 compare bytes: any alphabet, any length
    text = rng.integers(0, 20, 3000).astype(np.uint8)
    read = text[1000:1600].copy()
    read[[5, 300]] = (read[[5, 300]] + 1) % 20
    gp = V.Text.from_host(text, 20)
    gr = V.Queries.from_host(read, [0], [600])
    for mode in (OC.EXACT, OC.HAMMING):
        want = OM.findcompletematches(text, [read], mode, 3)
        assert np.array_equal(scan(V, gp, gr, mode, 3), want)
        assert len(want) == (mode == OC.HAMMING)
