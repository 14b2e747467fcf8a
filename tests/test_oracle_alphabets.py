"""The CPU oracle against the reference OFF the DNA alphabet: a protein
database under the 20-letter alphabet (mkvtree -protein), under an 11-class
symbol map (mkvtree -smap) and as an index that holds its queries -- fixtures
written by the real reference programs (scripts/make_golden_alphabets.py).
Table builder (oracle/vsindex.c) and every search of the oracle, bit-exact,
order included.  No GPU involved."""
import os

import numpy as np
import pytest

import alphabet_texts as A
import helpers as H

M = H.alphabets_manifest()


def parse_key(key):
    """run name -> (kind, L, keyword arguments of oracle_querymatches)"""
    name, _, sp = key.partition("_sp")
    for kind in ("selfmum", "supermax", "repeats", "tandem", "mumcand", "mum",
                 "mem"):
        if name.startswith(kind):
            kw = {"mumcand": dict(mum=True, cand=True), "mum": dict(mum=True),
                  "mem": dict(speedup=int(sp) if sp else 2)}.get(kind, {})
            return kind, int(name[len(kind):]), kw
    raise KeyError(key)


def run_oracle(idx, q, key):
    if key == "approx_e1":
        return H.matches_as_ref(idx, H.oracle_approx(idx, q, True, 1))
    if key == "complete":
        return H.matches_as_ref(idx, H.oracle_complete(idx, q))
    kind, L, kw = parse_key(key)
    if kind == "selfmum":
        return H.selfmatches_as_ref(idx, H.oracle_selfmum(idx, L))
    if kind == "repeats":
        conv = H.selfmatches_as_ref if idx.hasqueries else H.repeats_as_ref
        return conv(idx, H.oracle_repeats(idx, L))
    if kind == "supermax":
        return H.repeats_as_ref(idx, H.oracle_supermax(idx, L))
    if kind == "tandem":
        return H.repeats_as_ref(idx, H.oracle_tandems(idx, L))
    return H.matches_as_ref(idx, H.oracle_querymatches(idx, q, L, **kw))


def short_queries(idx):
    return H.fasta_queries(os.path.join(H.GOLDEN, "prot_short.fna"),
                           idx.symmap)


CASES = [(c, k) for c in sorted(M) for k in sorted(M[c]["runs"])]


def test_the_fixtures_cover_what_they_are_meant_to():
    assert sorted(M) == ["prot", "prot11", "prot_all"]
    assert M["prot"]["numofchars"] == 20 and M["prot11"]["numofchars"] == 11
    for case, key in CASES:
        run = M[case]["runs"][key]
        want = H.alphabets_expected(case, key)
        assert len(want) == run["lines"] > 0, (case, key)
        if key.startswith(("mem", "repeats")):
            assert 100 <= len(want) <= 100000, (case, key)
        assert "-p" not in run["args"]
    idx, q = H.load_alphabet_case("prot")
    assert idx.tis[0] < 20 and (idx.tis == H.WILDCARD).sum() > 20
    assert (q.symbols == H.WILDCARD).sum() >= 10


def test_symbol_map_from_al1_generalises_dna_map(tmp_path):
    p = str(tmp_path / "dna.al1")
    with open(p, "w") as f:
        f.write("aA\ncC\ngG\ntTuU\nnsywrkvbdhmNSYWRKVBDHM\n")
    assert np.array_equal(H.symbol_map_from_al1(p), H.dna_map())
    m = H.symbol_map_from_al1(os.path.join(H.GOLDEN, "prot11.al1"))
    # comment lines in front, display characters behind the blank
    assert m[ord("L")] == m[ord("F")] == 0 and m[ord("C")] == 10
    assert m[ord("X")] == m[ord("*")] == H.WILDCARD
    assert m[ord("i")] == 253 and m[ord("#")] == 253 and m[ord(" ")] == 253


@pytest.mark.parametrize("case", sorted(M))
def test_index_tables_match_reference_md5(case):
    """oracle/vsindex.c writes mkvtree's tables byte for byte at 20 and at 11
    symbols (load_alphabet_case asserts the md5 sums)"""
    idx, _ = H.load_alphabet_case(case)
    prj = M[case]["index"]["prj"]
    assert idx.n == prj["totallength"]
    assert idx.prefixlength == prj["prefixlength"] == \
        H.recommended_prefixlength(idx.numofchars, idx.n)
    assert idx.numofsequences == prj["numofsequences"]
    assert idx.nllv == prj["largelcpvalues"]


@pytest.mark.parametrize("case,key", CASES)
def test_oracle_reproduces_reference_output(case, key):
    run = M[case]["runs"][key]
    idx, q = H.load_alphabet_case(case)
    want = H.alphabets_expected(case, key)
    assert len(want) > 0
    if key == "complete_short":
        # the same message after the same partial list
        with pytest.raises(H.OracleError) as ei:
            H.oracle_complete(idx, short_queries(idx))
        assert run["rc"] != 0
        assert str(ei.value) == run["stderr"].split(": ", 1)[1]
        assert str(ei.value) == "patternlength=1 must be >= %d=prefixlen" % \
            idx.prefixlength
        got = H.matches_as_ref(idx, ei.value.partial)
    else:
        assert run["rc"] == 0
        got = run_oracle(idx, q, key)
    assert len(got) == run["lines"]
    # bit-exact INCLUDING the order in which the reference emits
    assert np.array_equal(got, want)


# ---- the seeded texts of tests/test_gpu_alphabets.py ------------------------


@pytest.mark.parametrize("nc", A.SWEEP)
def test_sweep_texts_give_no_empty_list(nc):
    """what the GPU tests compare against is never an empty list, at any
    alphabet size; the text has what it is meant to have"""
    c = A.sweep_case(nc)
    assert A.list_sizes(c) == A.SIZES[nc]
    for pl in c["index"]:                 # the same lists at either pl
        assert c["sizes"]["pl%d" % pl] == c["sizes"]["pl%d" % c["plrec"]]
    tis = c["tis"]
    assert len(tis) == 12002 and (tis == H.SEPARATOR).sum() == 2
    assert 10 <= (tis == H.WILDCARD).sum() <= 70
    assert tis[(tis < H.WILDCARD)].max() == nc - 1
    assert c["queries"].nq == 300
    assert c["queries"].length.min() >= max(c["index"])
    assert c["queries"].symbols[c["queries"].symbols < H.WILDCARD].max() < nc
    assert sorted(c["index"]) == sorted(
        {c["plrec"]} | ({A.forced_prefixlength(c["plrec"])} if nc >= 20
                        else set()))
    for pl, lists in c["query"].items():
        assert len(lists) == 1 + 4 * len(A.query_lengths(nc, pl))
        assert all(len(v) >= 200 for v in lists.values()), c["sizes"]
        assert max(len(v) for v in lists.values()) < 500000
    assert all(len(v) >= 7 for v in c["supermax"].values())
    assert len(c["tandem"][1]) >= 18 and len(c["tandem"][3]) > 0
    if nc <= A.REP_MAXC:
        assert len(c["repeats"][8]) >= len(c["repeats"][40]) >= 118
    if nc <= A.SELFMUM_MAXC:
        assert len(c["selfmum"]) > 0
    # the two algorithms of the reference report the same MEMs
    for pl, lists in c["query"].items():
        for L in A.query_lengths(nc, pl):
            if len(lists["mem_sp0%d" % L]) > 100000:
                continue                      # (sorting those takes seconds)
            assert np.array_equal(
                H.sorted_matches(lists["mem_sp0%d" % L]),
                H.sorted_matches(lists["mem_sp2%d" % L]))


def test_texts_for_many_classes_and_high_left_symbols():
    for nc, n in ((20, 946), (32, 1434)):
        tis = A.many_classes_text(nc)
        assert len(tis) == n
        idx = H.oracle_build_index(tis, nc, 1)
        sizes = [len(H.oracle_repeats(idx, L)) for L in (5, 10, 30)]
        assert sizes == {20: [465, 465, 55], 32: [1081, 1081, 105]}[nc]
        assert sizes[1] > nc * (nc - 1) // 2
        assert len(H.oracle_supermax(idx, 10)) >= 8
    nc, tis = A.high_left_symbols_text()
    idx = H.oracle_build_index(tis, nc)
    assert len(H.oracle_supermax(idx, 20)) == 4
    idx.bwt = np.where(idx.bwt < 253, idx.bwt & 63, idx.bwt).astype(np.uint8)
    assert len(H.oracle_supermax(idx, 20)) == 1
