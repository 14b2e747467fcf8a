"""vmatch -dnavsprot without a GPU: the host translation
(vsa_translate_host), the conversion of match records to DNA coordinates
(vsa_translated_convert_host) and the sink of kind VSA_SINK_TRANSLATED
reproduce what the real reference recorded
(tests/golden/translated_*, scripts/make_golden_translated.py): the amino acid
of every codon under every translation table, and byte for byte the stdout of
the runs on the protein database, the six-frame batch going through the CPU
oracle of the query engine."""
import numpy as np
import pytest

import helpers as H
import translated_cases as T


def translate_codons(V, transnum, codons):
    """-> (forward, reverse) letters of 3-character sequences"""
    dna = T.Dna(codons)
    sym, ps, pl = V.translate_host(transnum, dna.chars, dna.start, dna.length,
                                   T.amino_map())
    assert list(pl) == [1, 0, 0, 1, 0, 0] * len(codons)
    return (T.letters_of(sym[ps[0::6].astype(np.int64)]),
            T.letters_of(sym[ps[3::6].astype(np.int64)]))


@pytest.mark.parametrize("transnum", T.TABLES)
def test_plain_codons_of_every_table(V, transnum):
    """fixture (a): the position of the F / G line names the amino acid, no
    line is a stop codon"""
    assert T.TABLES == list(V.TRANSLATION_TABLES) and len(T.TABLES) == 17
    want = T.CODONS["plain"][str(transnum)]
    fwd, rev = translate_codons(V, transnum, T.codon_list(T.CODONS["bases"]))
    assert fwd == want["forward"] and rev == want["reverse"]
    assert "*" in fwd and len(set(fwd)) == 21


@pytest.mark.parametrize("transnum", [1, 2])
def test_wildcard_codons(V, transnum):
    """fixture (b): all 15^3 codons over TCAGNSYWRKVBDHM, and a lower-case /
    U sample"""
    want = T.CODONS["wildcards"][str(transnum)]
    cods = T.codon_list(T.CODONS["letters"])
    assert len(cods) == 3375
    fwd, rev = translate_codons(V, transnum, cods)
    assert fwd == want["forward"] and rev == want["reverse"]
    # the reproduced oddity: the base set of a wildcard is not complemented
    # in the reverse frames (ARA: K forward, Y in reverse under table 1)
    if transnum == 1:
        i = cods.index("ARA")
        assert (fwd[i], rev[i]) == ("K", "Y")
    sample = T.CODONS["sample"][str(transnum)]
    assert any("u" in c for c in sample["codons"])
    fwd, rev = translate_codons(V, transnum, sample["codons"])
    assert fwd == sample["forward"] and rev == sample["reverse"]


def test_frame_layout_for_lengths_0_to_8(V):
    """starts, lengths, separators, no trailing separator, empty frames"""
    rng = np.random.default_rng(5)
    symmap = T.amino_map()
    for n in list(range(9)) + [None]:
        lens = list(range(9)) if n is None else [n]
        dna = T.Dna(["".join("TCAG"[int(b)] for b in rng.integers(0, 4, k))
                     for k in lens])
        sym, ps, pl = V.translate_host(1, dna.chars, dna.start, dna.length,
                                       symmap)
        wps, wpl, total = T.expected_frames(dna.length)
        assert np.array_equal(ps, wps) and np.array_equal(pl, wpl)
        assert len(sym) == total
        issep = np.zeros(total, bool)
        issep[(wps + wpl)[:-1].astype(np.int64)] = True
        assert np.array_equal(sym == H.SEPARATOR, issep)
        assert total == 0 or sym[-1] != H.SEPARATOR or wpl[-1] == 0
        # every symbol is the codon the frame reads
        for s, seq in enumerate(dna.seqs):
            for f in range(3):
                got = T.letters_of(sym[int(ps[6 * s + f]):][:int(pl[6 * s + f])])
                cods = [seq[f + 3 * k:f + 3 * k + 3].decode()
                        for k in range(int(pl[6 * s + f]))]
                assert got == (translate_codons(V, 1, cods)[0] if cods else "")
    # an empty batch
    sym, ps, pl = V.translate_host(1, np.zeros(0, np.uint8), [], [], symmap)
    assert len(sym) == len(ps) == len(pl) == 0


def test_error_texts(V):
    for t, text in T.CODONS["errors"].items():
        with pytest.raises(V.VsaError) as e:
            V.transnum_check(int(t))
        assert e.value.code == -2
        assert e.value.message == text.split(": ", 1)[1]
        with pytest.raises(V.VsaError):
            V.translate_host(int(t), np.frombuffer(b"ACG", np.uint8), [0],
                             [3], T.amino_map())
    for t in T.TABLES:
        V.transnum_check(t)
    symmap = T.amino_map()
    # the first character the reference's order of frames and codons meets
    dna = T.Dna(["ACGT", "AC?", "ACGTTX", "??"])
    with pytest.raises(V.VsaError) as e:
        V.translate_host(1, dna.chars, dna.start, dna.length, symmap)
    assert (e.value.code, e.value.message) == (-2, "illegal char c2='?'(63)")
    # a sequence without a codon is not looked at
    dna = T.Dna(["ACGT", "??", "!"])
    V.translate_host(1, dna.chars, dna.start, dna.length, symmap)
    # an amino acid outside the alphabet of the map: the documented deviation
    symmap[ord("K")] = symmap[ord("k")] = 253
    with pytest.raises(V.VsaError) as e:
        V.translate_host(1, np.frombuffer(b"AAA", np.uint8), [0], [3], symmap)
    assert e.value.code == -2 and "amino acid 'K'" in e.value.message


_cache = {}


def case():
    if not _cache:
        idx, _ = H.load_alphabet_case("prot")
        _cache["idx"] = idx
        _cache["dna"] = T.Dna.fasta("translated_q.fna.gz")
        _cache["small"] = T.Dna.fasta("translated_complete.fna")
    return _cache["idx"], _cache["dna"], _cache["small"]


def oracle_list(V, key):
    idx, dna, _ = case()
    if ("list", key) not in _cache:
        transnum, kw = T.MATCH_RUNS[key]
        q = T.host_batch(V, dna, transnum, idx.symmap)
        _cache[("list", key)] = H.oracle_querymatches(idx, q, T.L, speedup=2,
                                                      **kw)
    return _cache[("list", key)]


def test_query_file_is_what_the_issue_asks_for():
    _, dna, small = case()
    assert 190 <= dna.nq <= 210 and int(dna.length.max()) <= 400
    assert {1, 2, 3, 4, 5} <= set(int(x) for x in dna.length)
    assert int(small.length.min()) >= 8


@pytest.mark.parametrize("key", sorted(T.MATCH_RUNS))
def test_recorded_stdout_of_the_match_runs(V, key):
    idx, dna, _ = case()
    assert T.RUNS[key]["rc"] == 0
    showmode = T.SHOW_ABSOLUTE if key == "mem_absolute" else 0
    got = T.sink(V, idx, dna, showmode).format(oracle_list(V, key))
    assert got == T.lines_of(key) and got.count(b"\n") >= 100
    assert b" F " in got and b" G " in got


def test_recorded_stdout_of_complete(V):
    idx, dna, small = case()
    q = T.host_batch(V, small, 1, idx.symmap)
    # (vmatch was run without -l: no least length)
    got = T.sink(V, idx, small, leastlength=0, complete=True).format(
        H.oracle_complete(idx, q))
    assert got == T.lines_of("complete")
    # the first frame shorter than the prefix length ends the run
    run = T.RUNS["complete_short"]
    with pytest.raises(H.OracleError) as e:
        H.oracle_complete(idx, T.host_batch(V, dna, 1, idx.symmap))
    assert str(e.value) == run["stderr"].split(": ", 1)[1]
    assert str(e.value) == "patternlength=0 must be >= 2=prefixlen"
    assert T.sink(V, idx, dna, leastlength=0, complete=True).format(
        e.value.partial) == \
        T.lines_of("complete_short")
    assert len(run["lines"]) >= 2


def test_recorded_nomatch_lines(V):
    idx, dna, _ = case()
    m = oracle_list(V, "mem")
    view, reverse = V.translated_convert_host(m, dna.length)
    assert reverse.any() and not reverse.all()
    assert np.array_equal(view["length"], 3 * m["length"])
    assert np.array_equal(view["queryseq"], m["queryseq"] // 6)
    assert np.array_equal(view["dbstart"], m["dbstart"])
    assert V.nomatch_format(T.query_runs(dna, view)) == \
        T.lines_of("mem_qnomatch")
    assert V.nomatch_format(T.database_runs(idx, m)) == \
        T.lines_of("mem_dbnomatch")
    # an offset counts six-frame sequences
    shifted = m.copy()
    shifted["queryseq"] += 6 * 1000
    v2, r2 = V.translated_convert_host(shifted, dna.length, offset=6000)
    assert np.array_equal(r2, reverse)
    assert np.array_equal(v2["queryseq"], view["queryseq"] + 1000)
    assert np.array_equal(v2["querystart"], view["querystart"])
    with pytest.raises(V.VsaError):
        V.translated_convert_host(shifted, dna.length, offset=6001)
    with pytest.raises(V.VsaError):
        V.translated_convert_host(shifted, dna.length, offset=0)


def test_kind_5_is_refused_by_select_cluster_and_chain(V):
    idx, dna, _ = case()
    m = oracle_list(V, "mum")
    lay = T.layout(V, idx, dna)
    for call in (lambda: V.select_host(lay, m, best=10),
                 lambda: V.cluster_host(lay, 50, 50, m),
                 lambda: V.chain_host(lay, m),
                 lambda: V.matchcluster_host(lay, V.MATCHCLUSTER_GAP, 10, m)):
        with pytest.raises(V.VsaError) as e:
            call()
        assert e.value.code == V.NOT_COVERED
