"""The constructed texts of the repeat family (repeat_cases.py) on the CPU:
the oracle against the recorded lists of the real reference
(tests/golden/repeat_edges_*, scripts/make_golden_repeat_edges.py), order
included; the definitional model (repeat_model.py) against the oracle as
sets; the situation each case exists for, on the host tables.  What
test_gpu_repeat_edges.py holds the kernels to is the oracle's list, so this
file is what makes that list the reference's and the definition's.

copies (44 850 pairs from one node) and runs (runs of thousands of one
symbol) are beyond the model's all-pairs groups: the model answers their
siblings copies_small and runs_small, built by the same builders; the full
sizes are held against the recorded reference."""
import hashlib
import json
import os
import shutil
import tempfile

import numpy as np
import pytest

import helpers as H
import repeat_cases as RC
import repeat_model as RM

with open(os.path.join(H.GOLDEN, "repeat_edges_manifest.json")) as _f:
    M = json.load(_f)
_expected = None

COLUMNS = ("length", "dbseq", "dbrel", "queryseq", "querystart")


def recorded(name, key):
    global _expected
    if _expected is None:
        _expected = np.load(os.path.join(H.GOLDEN,
                                         "repeat_edges_expected.npz"))
    return _expected["%s__%s" % (name, key)].astype(np.uint64)


def columns(m):
    return np.stack([m[k].astype(np.uint64) for k in COLUMNS],
                    axis=1).reshape(len(m), 5)


def md5_parsed(cols):
    return hashlib.md5(np.ascontiguousarray(cols, "<u8").tobytes()).hexdigest()


def test_every_case_is_recorded_or_modelled():
    assert set(RC.RECORDED) | set(RC.MODELLED) == set(RC.NAMES)
    assert sorted(M) == sorted(RC.RECORDED)
    # the full sizes the model leaves out have a sibling of the same builder
    for name in set(RC.NAMES) - set(RC.MODELLED):
        assert RC.SIBLING[name] in RC.MODELLED
        assert RC.case(name).lengths[-1] > 0
    for name in RC.RECORDED:
        assert sorted(M[name]["runs"]) == sorted(
            "%s%d" % r for r in RC.case(name).runs())


@pytest.mark.parametrize("name", RC.RECORDED)
def test_oracle_gives_the_recorded_reference_lists(name):
    c, m = RC.case(name), M[name]
    # builder and fixture have not drifted; the oracle's tables are the ones
    # the reference's mkvtree wrote
    assert c.md5() == m["md5_text"] and c.n == m["totallength"]
    assert c.host.prefixlength == m["prefixlength"]
    assert c.host.nllv == m["largelcpvalues"]
    assert H.table_md5(c.host) == m["md5_tables"]
    nonempty = 0
    for engine, L in c.runs():
        run = m["runs"]["%s%d" % (engine, L)]
        if run["rc"] != 0:
            with pytest.raises(H.OracleError) as e:
                c.oracle(engine, L)
            assert str(e.value) == run["stderr"]
            continue
        got = columns(c.as_ref(RC.expected(name, engine, L)))
        assert len(got) == run["lines"], (engine, L)
        assert md5_parsed(got) == run["md5_parsed"], (engine, L)
        if run["stored"]:
            assert np.array_equal(got, recorded(name, "%s%d" % (engine, L)))
        nonempty += len(got) > 0
    assert nonempty > 0 or c.n == 1


def test_a_text_of_one_symbol():
    """the reference's answers: an error for -l and -supermax, an empty list
    for -tandem"""
    runs = M["tiny_a"]["runs"]
    for key in ("repeats1", "repeats2", "supermax1", "supermax2"):
        assert runs[key]["rc"] != 0 and runs[key]["lines"] == 0
        assert runs[key]["stderr"] == \
            "repeat search requires a sequence of length >= 2"
    for key in ("tandem1", "tandem2"):
        assert runs[key]["rc"] == 0 and runs[key]["lines"] == 0
    assert len(RC.expected("tiny_a", "tandem", 1)) == 0


@pytest.mark.parametrize("name", RC.MODELLED)
def test_model_gives_the_oracles_sets(name):
    c = RC.case(name)
    kw = {"querysep": c.qsep} if c.hasqueries else {}
    for engine, L in c.runs():
        try:
            want = RC.expected(name, engine, L)
        except H.OracleError:
            assert c.n == 1
            continue
        got = RM.MODELS[engine](c.tis, L, **kw)
        assert len(got) == len(want), (engine, L)       # no pair twice
        assert got == RM.as_set(want), (engine, L)


@pytest.mark.parametrize("name", RC.NAMES)
def test_cases_hold_their_situations(name):
    RC.case(name).check_situation()


def test_candidate_rule_counts_on_a_known_table():
    """RC.candidates on lcp bytes written out by hand: 0 3 3 255 2 255 255 0"""
    class T:
        n = 7
        lcp = np.array([0, 3, 3, 255, 2, 255, 255, 0], np.uint8)
    assert RC.candidates(T, "repeats", 3) == 5
    assert RC.candidates(T, "repeats", 4) == 3
    assert RC.candidates(T, "tandem", 300) == 3
    assert RC.candidates(T, "repeats", 1) == 6
    # rises at positions 0 (first), 2 (3 < 255), 4 (2 < 255); 5: byte of 255
    assert RC.candidates(T, "supermax", 3) == 4
    assert RC.candidates(T, "supermax", 255) == 3


@pytest.mark.skipif(not H.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("name", RC.RECORDED)
def test_live_reference_prints_the_recorded_lists(name):
    c, m = RC.case(name), M[name]
    wd = tempfile.mkdtemp()
    try:
        recs = c.records()
        if c.hasqueries:
            H.write_fasta(wd + "/db.fna", recs[:c.numofdbsequences])
            H.write_fasta(wd + "/q.fna", recs[c.numofdbsequences:])
        else:
            H.write_fasta(wd + "/db.fna", recs)
        H.run_mkvtree_ref(m["mkvargs"], wd)
        ref = H.load_mkvtree_index(os.path.join(wd, m["indexname"]))
        assert H.table_md5(ref) == m["md5_tables"]
        for key, run in sorted(m["runs"].items()):
            rc, lines, err = H.run_vmatch_ref(run["args"], wd)
            assert rc == run["rc"] and len(lines) == run["lines"], key
            assert hashlib.md5(("\n".join(lines) + "\n").encode()
                               ).hexdigest() == run["md5_lines"], key
            if rc != 0:
                assert err.split(": ", 1)[1].strip() == run["stderr"]
    finally:
        shutil.rmtree(wd)
