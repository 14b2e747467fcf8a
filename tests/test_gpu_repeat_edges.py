"""The repeat family on the GPU (vmatch -l L IDX, -supermax, -tandem;
vstree_amd/csrc/selfmatch_search.inc) on the constructed texts of
repeat_cases.py: lcp exceptions in rows around a node's depth with search
lengths on both sides of 255, one node of 300 suffixes whose left characters
are all special, attachments with every left-character class on both sides,
depths of thousands, texts of 1 .. 33 symbols.

Every list must be the CPU oracle's, order included;
test_repeat_model_host.py holds those lists to the recorded output of the
real reference and to the definitions.  Every search runs on an index built
on the GPU and on one uploaded from the CPU builder's tables, each on 32-bit
and (VSA_FORCE_WIDE=1) 64-bit device tables; tandems also with
VSA_TANDEM_ISA=1.  The number of candidates the selection kernels report is
held to the rule of lcpsel_mask evaluated on the host's lcp bytes.  All
values are integers: equal or wrong."""
import numpy as np
import pytest

import helpers as H
import repeat_cases as RC
import test_repeat_model_host as TH
from test_gpu_approx_edges import env

pytestmark = pytest.mark.gpu

SEARCH = {"repeats": "findmaximalrepeats",
          "supermax": "findsupermaximalrepeats", "tandem": "findtandems"}


def make_indexes(V, c):
    """[(label, index)]: built on the GPU | from the CPU builder's tables, on
    32-bit | 64-bit device tables (the library reads VSA_FORCE_WIDE when an
    index is made).  The built tables must be the host's: the situation of
    the case, checked on the host's tables, is then the GPU's, too."""
    made = []
    for wide in (False, True):
        host = c.host.as_width(64 if wide else 32)
        with env("VSA_FORCE_WIDE", wide):
            built = V.Index.build(c.tis, 4, 0)
            tables = V.Index.from_tables(
                host.n, host.prefixlength, 4, host.tis, host.suf, host.lcp,
                host.llv, host.bck, host.bwt, host.querysepposition,
                host.hasqueries)
        if c.hasqueries:
            built.set_queryseparator(c.qsep)
        got = built.download()
        for k in ("tis", "suf", "lcp", "llv", "bwt"):
            assert np.array_equal(got[k].astype(np.uint64),
                                  getattr(host, k).astype(np.uint64)), k
        for how, gi in (("built", built), ("tables", tables)):
            info = gi.info()
            assert info.device_integersize == (64 if wide else 32)
            assert info.prefixlength == host.prefixlength
            assert info.largelcpvalues == host.nllv
            assert info.hasindexedqueries == int(c.hasqueries)
            made.append(("%s/%s" % (how, "wide" if wide else "narrow"), gi))
    return made


_gpu = {}


def indexes(V, c):
    if c.name not in _gpu:
        _gpu[c.name] = make_indexes(V, c)
    return _gpu[c.name]


def forms(engine):
    """(label, VSA_TANDEM_ISA) of the forms an engine has"""
    if engine == "tandem":
        return (("text", False), ("isa", True))
    return (("", False),)


def search(V, gi, engine, L, isa=False):
    with env("VSA_TANDEM_ISA", isa):
        return getattr(V, SEARCH[engine])(gi, L)


def refusal(name, engine, L):
    """the reference's error text where it refuses the search, else None"""
    run = TH.M[name]["runs"]["%s%d" % (engine, L)] if name in TH.M else None
    return run["stderr"] if run is not None and run["rc"] != 0 else None


# nothing to find at any length: the texts made for the other two engines,
# and two sequences of one symbol, hold no square
NOTHING = {("copies", "tandem"), ("copies_small", "tandem"),
           ("nested", "tandem"), ("star", "tandem"), ("tiny_a_a", "tandem")}


@pytest.mark.parametrize("name,engine", [(n, e) for n in RC.NAMES
                                         for e in RC.case(n).engines])
def test_every_search_gives_the_oracles_list(V, name, engine):
    c = RC.case(name)
    c.check_situation()
    records = 0
    for iname, gi in indexes(V, c):
        for L in c.lengths:
            message = refusal(name, engine, L)
            for fname, isa in forms(engine):
                form = (name, iname, engine, L, fname)
                if message is not None:
                    with pytest.raises(V.VsaError) as e:
                        search(V, gi, engine, L, isa)
                    assert e.value.message == message, form
                    continue
                want = RC.expected(name, engine, L)
                res = search(V, gi, engine, L, isa)
                got, st = res.fetch(), res.stats()
                assert len(got) == len(want), form + (len(got), len(want))
                assert np.array_equal(got, want), form
                assert st.count == len(want), form
                assert st.candidates == RC.candidates(c.host, engine, L), \
                    form + (st.candidates,)
                records += len(got)
    assert (records > 0) == (c.n > 1 and (name, engine) not in NOTHING)


def test_a_text_of_one_symbol(V):
    """the reference refuses -l and -supermax on it and answers -tandem with
    an empty list (tests/golden/repeat_edges_manifest.json, tiny_a)"""
    c = RC.case("tiny_a")
    assert c.n == 1
    message = "repeat search requires a sequence of length >= 2"
    for iname, gi in indexes(V, c):
        for L in (1, 2):
            for fn in (V.findmaximalrepeats, V.findsupermaximalrepeats):
                assert refusal("tiny_a", "repeats", L) == message
                with pytest.raises(V.VsaError) as e:
                    fn(gi, L)
                assert e.value.message == message, (iname, L)
            for fname, isa in forms("tandem"):
                res = search(V, gi, "tandem", L, isa)
                assert res.count == 0 and len(res.fetch()) == 0
                assert res.stats().candidates == 0


@pytest.mark.parametrize("name,L", [("runs", 300), ("runs_tail", 255),
                                    ("nested_tandem", 254),
                                    ("nested", 255), ("star", 10)])
def test_three_calls_in_a_row_answer_alike(V, name, L):
    """on an index of its own, so that the first tandem call with
    VSA_TANDEM_ISA=1 is the one that builds the inverse suffix array"""
    c = RC.case(name)
    for wide in (False, True):
        with env("VSA_FORCE_WIDE", wide):
            gi = V.Index.build(c.tis, 4, 0)
        for engine in c.engines:
            want = RC.expected(name, engine, L)
            for fname, isa in reversed(forms(engine)):
                for call in range(3):
                    got = search(V, gi, engine, L, isa).fetch()
                    assert len(got) == len(want), (engine, fname, call)
                    assert np.array_equal(got, want), (engine, fname, call)
    assert len(RC.expected(name, c.engines[0], L)) > 0
