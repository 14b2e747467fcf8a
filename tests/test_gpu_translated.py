"""vmatch -dnavsprot on the GPU: the translation kernel writes byte for byte
what vsa_translate_host writes -- symbols, starts and lengths -- at the
smallest shapes at which it can go wrong (every length around a frame and
around the kernel's tile, sequences that straddle workgroups, a long
sequence, every wildcard codon, the uniform device form), its errors leave no
batch behind, and the recorded runs of the real reference
(tests/golden/translated_*) come out of Queries.translate -> query engine ->
sink, conversion and coverage as they do out of the host path."""
import numpy as np
import pytest

import helpers as H
import translated_cases as T

pytestmark = pytest.mark.gpu

TILE = 256  # == V.TRANSLATE_TILE, asserted below


def random_dna(rng, n, wildcards=0.0):
    s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy()
    if wildcards:
        hit = rng.random(n) < wildcards
        s[hit] = np.frombuffer(b"NSYWRKVBDHMnu", np.uint8)[
            rng.integers(0, 13, int(hit.sum()))]
    return s.tobytes()


def same_as_host(V, dna, transnum=1, symmap=None):
    symmap = T.amino_map() if symmap is None else symmap
    sym, ps, pl = V.translate_host(transnum, dna.chars, dna.start, dna.length,
                                   symmap)
    q = V.Queries.translate(transnum, dna.chars, dna.start, dna.length, symmap)
    info = q.info()
    assert info.numofqueries == 6 * dna.nq == q.nq
    assert info.numofsymbols == len(sym)
    gsym, gps, gpl = q.download()
    assert np.array_equal(gps, ps) and np.array_equal(gpl, pl)
    assert np.array_equal(gsym, sym)
    if dna.nq:
        assert (info.minlength, info.maxlength) == (int(pl.min()),
                                                    int(pl.max()))
    return q


def test_tile_constant(V):
    assert V.TRANSLATE_TILE == TILE == int(V.lib.vsa_translate_tile())


def test_empty_batch(V):
    q = same_as_host(V, T.Dna([]))
    assert q.info().numofsymbols == 0


@pytest.mark.parametrize("n", range(9))
def test_one_sequence_of_each_small_length(V, n):
    rng = np.random.default_rng(100 + n)
    same_as_host(V, T.Dna([random_dna(rng, n)]))
    same_as_host(V, T.Dna([random_dna(rng, n, 0.3)]), transnum=2)


@pytest.mark.parametrize("n", [3 * TILE - 1, 3 * TILE, 3 * TILE + 1,
                               3 * TILE + 2, 2 * 3 * TILE + 1])
def test_lengths_around_the_tile(V, n):
    rng = np.random.default_rng(n)
    same_as_host(V, T.Dna([random_dna(rng, n, 0.05)]))
    # ... and with a neighbour on either side
    same_as_host(V, T.Dna([random_dna(rng, 7), random_dna(rng, n, 0.05),
                           random_dna(rng, 11)]), transnum=11)


def test_sequences_straddle_workgroups(V):
    """short sequences, several per workgroup, of every length 0 .. 40, one
    workgroup whose every slot is a sequence of its own, and sequences of a
    few tiles between them"""
    rng = np.random.default_rng(7)
    seqs = [random_dna(rng, int(n), 0.05) for n in rng.integers(0, 41, 600)]
    seqs += [random_dna(rng, 3 + int(n)) for n in rng.integers(0, 3, 700)]
    seqs += [random_dna(rng, int(n), 0.02)
             for n in rng.integers(2 * TILE, 9 * TILE, 12)]
    order = rng.permutation(len(seqs))
    same_as_host(V, T.Dna([seqs[i] for i in order]), transnum=4)
    # 700 sequences of one slot each, in a row: more than a tile of them
    same_as_host(V, T.Dna(seqs[600:1300]))


def test_one_sequence_of_a_million_characters(V):
    rng = np.random.default_rng(8)
    same_as_host(V, T.Dna([random_dna(rng, 1000003, 0.01)]))


@pytest.mark.parametrize("transnum", [1, 2])
def test_wildcard_codons(V, transnum):
    cods = T.codon_list(T.CODONS["letters"])
    q = same_as_host(V, T.Dna(cods), transnum)
    sym, ps, _ = q.download()
    want = T.CODONS["wildcards"][str(transnum)]
    assert T.letters_of(sym[ps[0::6].astype(np.int64)]) == want["forward"]
    assert T.letters_of(sym[ps[3::6].astype(np.int64)]) == want["reverse"]


@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 100])
def test_uniform_reads_in_device_memory(V, m):
    rng = np.random.default_rng(m)
    nq = 1000
    chars = np.frombuffer(random_dna(rng, nq * m, 0.02), np.uint8)
    symmap = T.amino_map()
    start = np.arange(nq, dtype=np.uint64) * np.uint64(m)
    length = np.full(nq, m, np.uint64)
    sym, ps, pl = V.translate_host(1, chars, start, length, symmap)
    d = V.device_malloc(nq * m)
    try:
        V.device_upload(d, chars)
        q = V.Queries.translate_device(1, d, nq, m, symmap)
        gsym, gps, gpl = q.download()
        assert np.array_equal(gps, ps) and np.array_equal(gpl, pl)
        assert np.array_equal(gsym, sym)
        # the reads are still what they were
        back = np.zeros(nq * m, np.uint8)
        V.device_download(back, d)
        assert np.array_equal(back, chars)
    finally:
        V.device_free(d)


def test_errors_leave_no_batch(V):
    symmap = T.amino_map()
    rng = np.random.default_rng(9)
    seqs = [random_dna(rng, 50) for _ in range(40)]
    seqs[17] = seqs[17][:31] + b"?" + seqs[17][32:]
    seqs[30] = seqs[30][:5] + b"!" + seqs[30][6:]
    dna = T.Dna(seqs)
    with pytest.raises(V.VsaError) as host:
        V.translate_host(1, dna.chars, dna.start, dna.length, symmap)
    with pytest.raises(V.VsaError) as e:
        V.Queries.translate(1, dna.chars, dna.start, dna.length, symmap)
    assert (e.value.code, e.value.message) == (-2, host.value.message)
    assert e.value.message == "illegal char c1='?'(63)"
    # a sequence without a codon is not looked at
    same_as_host(V, T.Dna([b"ACGT", b"??", b"!"]))
    # the uniform form
    m, nq = 50, 40
    chars = np.frombuffer(b"".join(seqs), np.uint8)
    d = V.device_malloc(nq * m)
    try:
        V.device_upload(d, chars)
        with pytest.raises(V.VsaError) as e:
            V.Queries.translate_device(1, d, nq, m, symmap)
        assert (e.value.code, e.value.message) == (-2, host.value.message)
    finally:
        V.device_free(d)
    # an amino acid the map of the index does not know
    symmap[ord("K")] = symmap[ord("k")] = 253
    dna = T.Dna([random_dna(rng, 60) for _ in range(30)] + [b"CCAAAGG"])
    with pytest.raises(V.VsaError) as host:
        V.translate_host(1, dna.chars, dna.start, dna.length, symmap)
    with pytest.raises(V.VsaError) as e:
        V.Queries.translate(1, dna.chars, dna.start, dna.length, symmap)
    assert (e.value.code, e.value.message) == (-2, host.value.message)
    assert "amino acid 'K'" in e.value.message
    with pytest.raises(V.VsaError) as e:
        V.Queries.translate(7, dna.chars, dna.start, dna.length, symmap)
    assert e.value.message == T.CODONS["errors"]["7"].split(": ", 1)[1]


# ---- the recorded runs -------------------------------------------------------

_cache = {}


def case(V):
    if not _cache:
        idx, _ = H.load_alphabet_case("prot")
        _cache["idx"] = idx
        _cache["gi"] = V.Index.from_tables(
            idx.n, idx.prefixlength, idx.numofchars, idx.tis, idx.suf,
            idx.lcp, idx.llv, idx.bck, idx.bwt)
        _cache["dna"] = T.Dna.fasta("translated_q.fna.gz")
        _cache["small"] = T.Dna.fasta("translated_complete.fna")
    return _cache["idx"], _cache["gi"], _cache["dna"], _cache["small"]


def batch(V, transnum):
    idx, _, dna, _ = case(V)
    if ("batch", transnum) not in _cache:
        _cache[("batch", transnum)] = V.Queries.translate(
            transnum, dna.chars, dna.start, dna.length, idx.symmap)
    return _cache[("batch", transnum)]


def gpu_list(V, key):
    """-> (Result, its records) of a recorded match run"""
    _, gi, _, _ = case(V)
    if ("list", key) not in _cache:
        transnum, kw = T.MATCH_RUNS[key]
        r = V.findquerymatches(gi, batch(V, transnum), T.L, speedup=2, **kw)
        _cache[("list", key)] = (r, r.fetch())
    return _cache[("list", key)]


@pytest.mark.parametrize("key", sorted(T.MATCH_RUNS))
def test_recorded_stdout_of_the_match_runs(V, key):
    idx, _, dna, _ = case(V)
    showmode = T.SHOW_ABSOLUTE if key == "mem_absolute" else 0
    got = T.sink(V, idx, dna, showmode).format(gpu_list(V, key)[1])
    assert got == T.lines_of(key) and got.count(b"\n") >= 100


def test_recorded_stdout_of_complete(V):
    idx, gi, dna, small = case(V)
    q = V.Queries.translate(1, small.chars, small.start, small.length,
                            idx.symmap)
    got = T.sink(V, idx, small, leastlength=0, complete=True).format(
        V.findcompletematches(gi, q).fetch())
    assert got == T.lines_of("complete")
    run = T.RUNS["complete_short"]
    with pytest.raises(V.VsaError) as e:
        V.findcompletematches(gi, batch(V, 1))
    assert e.value.message == run["stderr"].split(": ", 1)[1]
    assert T.sink(V, idx, dna, leastlength=0, complete=True).format(
        e.value.partial.fetch()) == T.lines_of("complete_short")


@pytest.mark.parametrize("key", ["mem", "mum", "mem_table4"])
def test_conversion_equals_the_host_conversion(V, key):
    _, _, dna, _ = case(V)
    r, m = gpu_list(V, key)
    view, reverse = V.translated_convert(r, batch(V, T.MATCH_RUNS[key][0]))
    hview, hreverse = V.translated_convert_host(m, dna.length)
    assert len(m) >= 100 and reverse.any() and not reverse.all()
    assert np.array_equal(view.fetch(), hview)
    assert np.array_equal(reverse, hreverse)


def test_conversion_with_an_offset_and_its_refusals(V):
    idx, gi, dna, _ = case(V)
    q = V.Queries.translate(1, dna.chars, dna.start, dna.length, idx.symmap)
    _, m = gpu_list(V, "mem")
    q.set_offset(6 * 1000)
    r = V.findquerymatches(gi, q, T.L, speedup=2)
    view, reverse = V.translated_convert(r, q)
    hview, hreverse = V.translated_convert_host(m, dna.length)
    hview["queryseq"] += 1000
    assert np.array_equal(view.fetch(), hview)
    assert np.array_equal(reverse, hreverse)
    q.set_offset(6001)
    with pytest.raises(V.VsaError) as e:
        V.translated_convert(r, q)
    assert e.value.code == -2 and "multiple of 6" in e.value.message
    # a batch that is not a translation, a packed-pair list
    plain = V.Queries.from_host(np.zeros(8, np.uint8), [0], [8])
    with pytest.raises(V.VsaError) as e:
        V.translated_convert(gpu_list(V, "mem")[0], plain)
    assert e.value.code == -2
    packed = V.findmumcandidates_packed(gi, batch(V, 1), T.L)
    with pytest.raises(V.VsaError) as e:
        V.translated_convert(packed, batch(V, 1))
    assert e.value.code == V.NOT_COVERED


def test_coverage_from_the_query_view_and_the_database_side(V):
    idx, gi, dna, _ = case(V)
    r, m = gpu_list(V, "mem")
    view, _ = V.translated_convert(r, batch(V, 1))
    # the DNA batch of the coverage: only its lengths play a role
    codes = H.dna_map()[dna.chars]
    codes[dna.chars == 255] = H.SEPARATOR
    dq = V.Queries.from_host(codes, dna.start, dna.length)
    cov = V.Coverage.over_queries(dq)
    assert cov.nbits == dna.totallength
    cov.mark(view, layout=V.COVERAGE_QUERY, side=V.COVERAGE_QUERIES)
    assert V.nomatch_format(cov.nomatch(T.NOMATCH)) == \
        T.lines_of("mem_qnomatch")
    cov = V.Coverage.over_index(gi)
    cov.mark(r, layout=V.COVERAGE_QUERY, side=V.COVERAGE_DATABASE)
    assert V.nomatch_format(cov.nomatch(T.NOMATCH)) == \
        T.lines_of("mem_dbnomatch")


def test_kind_5_is_refused_on_the_device(V):
    idx, _, dna, _ = case(V)
    lay = T.layout(V, idx, dna)
    for make in (lambda: V.Select(lay, best=10),
                 lambda: V.Cluster(lay, 50, 50),
                 lambda: V.MatchCluster(lay, V.MATCHCLUSTER_GAP, 10),
                 lambda: V.Chain(lay)):
        with pytest.raises(V.VsaError) as e:
            make()
        assert e.value.code == V.NOT_COVERED
