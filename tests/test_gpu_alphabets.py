"""Exact matching and the repeat family OFF the DNA alphabet: the paths that
run only (or differently) when numofchars != 4 -- the generic q-gram code, the
reference form of every search stage (no derived tables), maximal repeats
with up to 32 left-character classes, the 256-bit left-symbol set of
supermaximal repeats, the builder's symbol packing at alphabet sizes next to
powers of two.

Against the golden lists of the real reference on a protein database
(scripts/make_golden_alphabets.py) and against the CPU oracle, which
tests/test_oracle_alphabets.py holds to the same golden lists.  Integer match
lists and table bytes: bit-exact, order included; no comparison of two empty
lists."""
import gzip
import hashlib
import os
import shutil

import numpy as np
import pytest

import alphabet_texts as A
import helpers as H
from test_gpu_dropin import needs_binaries, run_gpu_vmatch
from test_gpu_pipeline import run_job
from test_oracle_alphabets import parse_key

pytestmark = pytest.mark.gpu
M = H.alphabets_manifest()


def force_wide(on):
    """context: VSA_FORCE_WIDE=1 while an index is created (the library reads
    the switch there), as test_gpu_parity.gpu_index does"""
    class Ctx:
        def __enter__(self):
            self.before = os.environ.get("VSA_FORCE_WIDE")
            if on:
                os.environ["VSA_FORCE_WIDE"] = "1"

        def __exit__(self, *exc):
            if on:
                if self.before is None:
                    del os.environ["VSA_FORCE_WIDE"]
                else:
                    os.environ["VSA_FORCE_WIDE"] = self.before
    return Ctx()


def upload(V, idx, bits=64, wide=False):
    i = idx.as_width(bits)
    with force_wide(wide):
        gi = V.Index.from_tables(i.n, i.prefixlength, i.numofchars, i.tis,
                                 i.suf, i.lcp, i.llv, i.bck, i.bwt,
                                 i.querysepposition, i.hasqueries)
    info = gi.info()
    if wide:
        assert info.device_integersize == 64
    # no derived tables off DNA: every search stage runs in its reference form
    assert info.deepprefix == 0 and info.numofchars == idx.numofchars
    return gi


def gpu_queries(V, q):
    return V.Queries.from_host(q.symbols, q.start, q.length)


def same(got, want, least=1):
    """bit-exact, order included, and never two empty lists"""
    assert len(want) >= least, (len(want), least)
    assert len(got) == len(want), (len(got), len(want))
    assert np.array_equal(got, want)


# ---- a. the golden lists of the reference ----------------------------------

VARIANTS = {"tables64": (64, False), "tables32": (32, False),
            "wide": (64, True)}
_golden = {}


def golden_index(V, case, variant):
    if (case, variant) not in _golden:
        idx, _ = H.load_alphabet_case(case)
        _golden[(case, variant)] = upload(V, idx, *VARIANTS[variant])
    return _golden[(case, variant)]


def run_gpu(V, gi, idx, q, key):
    if key == "complete":
        return H.matches_as_ref(
            idx, V.findcompletematches(gi, gpu_queries(V, q)).fetch())
    kind, L, kw = parse_key(key)
    if kind == "selfmum":
        return H.selfmatches_as_ref(
            idx, V.findmaximaluniquematches(gi, L).fetch())
    if kind == "repeats":
        conv = H.selfmatches_as_ref if idx.hasqueries else H.repeats_as_ref
        return conv(idx, V.findmaximalrepeats(gi, L).fetch())
    if kind == "supermax":
        return H.repeats_as_ref(idx, V.findsupermaximalrepeats(gi, L).fetch())
    if kind == "tandem":
        return H.repeats_as_ref(idx, V.findtandems(gi, L).fetch())
    kw = dict(kw)
    kw.setdefault("speedup", 2)
    return H.matches_as_ref(
        idx, V.findquerymatches(gi, gpu_queries(V, q), L, **kw).fetch())


GOLDEN_RUNS = [(c, k) for c in sorted(M) for k in sorted(M[c]["runs"])
               if not k.startswith("approx_")]


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("case,key", GOLDEN_RUNS)
def test_gpu_reproduces_reference_output(V, case, key, variant):
    idx, q = H.load_alphabet_case(case)
    gi = golden_index(V, case, variant)
    want = H.alphabets_expected(case, key)
    if key == "complete_short":
        # the reference's hard error after the matches of the reads in front
        short = H.fasta_queries(os.path.join(H.GOLDEN, "prot_short.fna"),
                                idx.symmap)
        with pytest.raises(V.VsaError) as e:
            V.findcompletematches(gi, gpu_queries(V, short))
        assert e.value.message == \
            M[case]["runs"][key]["stderr"].split(": ", 1)[1]
        got = H.matches_as_ref(idx, e.value.partial.fetch())
    else:
        got = run_gpu(V, gi, idx, q, key)
    same(got, want)


# ---- b. the builder ----------------------------------------------------------

def md5s(t):
    return {k: hashlib.md5(np.ascontiguousarray(t[k]).astype(
        np.uint64 if k in ("suf", "llv", "bck") else np.uint8).tobytes()
    ).hexdigest() for k in ("tis", "suf", "lcp", "llv", "bck", "bwt")}


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("case", sorted(M))
def test_built_tables_have_the_references_md5(V, case, wide):
    idx, _ = H.load_alphabet_case(case)
    with force_wide(wide):
        gi = V.Index.build(idx.tis, idx.numofchars, idx.prefixlength)
        rec = V.Index.build(idx.tis, idx.numofchars, 0)
    info = gi.info()
    assert info.device_integersize == (64 if wide else 32)
    assert info.deepprefix == 0
    got = md5s(gi.download())
    assert got == {k: M[case]["index"]["md5"][k] for k in got}
    assert info.largelcpvalues == M[case]["index"]["prj"]["largelcpvalues"]
    assert rec.info().prefixlength == M[case]["index"]["prj"]["prefixlength"]


# ---- c. alphabet sweep against the oracle ------------------------------------

_built = {}


def built_index(V, nc, pl):
    """index of the sweep text built ON THE GPU, its tables checked against
    the oracle's"""
    if (nc, pl) not in _built:
        c = A.sweep_case(nc)
        want = c["index"][pl]
        gi = V.Index.build(c["tis"], nc, pl)
        info = gi.info()
        assert info.deepprefix == 0 and info.prefixlength == pl
        assert info.numofcodes == nc ** pl
        got = gi.download()
        for k in ("tis", "suf", "lcp", "llv", "bck", "bwt"):
            assert np.array_equal(got[k].astype(np.uint64),
                                  getattr(want, k).astype(np.uint64)), k
        _built[(nc, pl)] = gi
    return _built[(nc, pl)]


SWEEP_PL = [(nc, which) for nc in A.SWEEP
            for which in ("recommended", "forced")
            if which == "recommended" or nc >= 20]


@pytest.mark.parametrize("nc,which", SWEEP_PL)
def test_sweep_query_matching(V, nc, which):
    c = A.sweep_case(nc)
    pl = (c["plrec"] if which == "recommended"
          else A.forced_prefixlength(c["plrec"]))
    if which == "recommended":
        gi0 = V.Index.build(c["tis"], nc, 0)
        assert gi0.info().prefixlength == c["plrec"]
    assert pl in c["index"]
    gi = built_index(V, nc, pl)
    gq = gpu_queries(V, c["queries"])
    want = c["query"][pl]
    # list sizes on these texts (the oracle's, all 18 alphabets): -complete
    # 211 .. 435, MUM 213 .. 393, candidates and MEM above that
    same(V.findcompletematches(gi, gq).fetch(), want["complete"], least=200)
    for L in A.query_lengths(nc, pl):
        for name, kw in A.MODES:
            same(V.findquerymatches(gi, gq, L, **kw).fetch(),
                 want["%s%d" % (name, L)], least=200)


@pytest.mark.parametrize("nc", A.SWEEP)
def test_sweep_repeat_family(V, nc):
    c = A.sweep_case(nc)
    gi = built_index(V, nc, c["plrec"])
    for L in (3, 8, 40):
        same(V.findsupermaximalrepeats(gi, L).fetch(), c["supermax"][L],
             least=7)
    same(V.findtandems(gi, 1).fetch(), c["tandem"][1], least=18)
    same(V.findtandems(gi, 3).fetch(), c["tandem"][3])
    if nc <= A.REP_MAXC:
        same(V.findmaximalrepeats(gi, 8).fetch(), c["repeats"][8])
        same(V.findmaximalrepeats(gi, 40).fetch(), c["repeats"][40],
             least=118)
    else:
        for L in (8, 40):
            with pytest.raises(V.VsaError) as e:
                V.findmaximalrepeats(gi, L)
            assert e.value.code == V.NOT_COVERED
            assert "not covered" in e.value.message


@pytest.mark.parametrize("nc", A.SWEEP)
def test_sweep_self_mum_scan(V, nc):
    c = A.sweep_case(nc)
    gi = V.Index.build(c["selftis"], nc, c["plrec"])
    gi.set_queryseparator(c["selfsep"])
    assert gi.info().hasindexedqueries == 1
    if nc <= A.SELFMUM_MAXC:
        got = gi.download()
        for k in ("suf", "lcp", "bwt"):
            assert np.array_equal(got[k].astype(np.uint64), getattr(
                c["selfindex"], k).astype(np.uint64)), k
        same(V.findmaximaluniquematches(gi, 8).fetch(), c["selfmum"])
    else:
        with pytest.raises(V.VsaError) as e:
            V.findmaximaluniquematches(gi, 8)
        assert e.value.code == V.NOT_COVERED
        assert "not covered" in e.value.message


def astuples(m):
    return [tuple(int(x) for x in r) for r in m.tolist()]


def test_callback_variants_deliver_the_same_lists(V):
    nc = 20
    c = A.sweep_case(nc)
    pl = c["plrec"]
    gi, gq = built_index(V, nc, pl), gpu_queries(V, c["queries"])
    want = c["query"][pl]
    rc, got = V.findcompletematches_cb(gi, gq)
    assert rc == 0 and len(got) > 0 and got == astuples(want["complete"])
    L = A.query_lengths(nc, pl)[-1]
    for name, kw in A.MODES:
        rc, got = V.findquerymatches_cb(gi, gq, L, **kw)
        w = astuples(want["%s%d" % (name, L)])
        assert rc == 0 and len(w) > 0 and got == w, name
    si = V.Index.build(c["selftis"], nc, pl)
    si.set_queryseparator(c["selfsep"])
    rc, got = V.findmaximaluniquematches_cb(si, 8)
    assert rc == 0 and len(got) > 0 and got == astuples(c["selfmum"])


def test_approximate_matching_declines_a_protein_sized_alphabet(V):
    c = A.sweep_case(20)
    gi, gq = built_index(V, 20, c["plrec"]), gpu_queries(V, c["queries"])
    for doedist, k, percent in ((True, 1, 0), (False, 1, 0), (True, 5, 1),
                                (True, 5, 2)):
        with pytest.raises(V.VsaError) as e:
            V.findapproxcompletematches(gi, gq, doedist, k, percent)
        assert e.value.code == V.NOT_COVERED
        assert "not covered" in e.value.message
        assert e.value.partial is None
    rc, got = V.findapproxcompletematches_cb(gi, gq, True, 1)
    assert rc == V.NOT_COVERED and got == []


# ---- d. maximal repeats with many left-character classes at one node ---------

@pytest.mark.parametrize("nc", [20, 32])
def test_maximal_repeats_with_many_left_character_classes(V, nc):
    tis = A.many_classes_text(nc)
    idx = H.oracle_build_index(tis, nc, 1)
    for gi in (upload(V, idx), V.Index.build(tis, nc, 1)):
        for L in (5, 10, 30):
            want = H.oracle_repeats(idx, L)
            # one node whose father and son lists hold every class: more
            # pairs than there are pairs of classes
            same(V.findmaximalrepeats(gi, L).fetch(), want,
                 least=nc * (nc - 1) // 2 + 1 if L == 10 else 1)
            same(V.findsupermaximalrepeats(gi, L).fetch(),
                 H.oracle_supermax(idx, L))


# ---- e. supermaximal repeats, left symbols that differ only above bit 5 ------

def test_supermaximal_repeats_tell_left_symbols_64_apart(V):
    nc, tis = A.high_left_symbols_text()
    idx = H.oracle_build_index(tis, nc)
    want = H.oracle_supermax(idx, 20)
    # the three pairs of V (left symbols 5, 69, 133) and [70] W
    assert astuples(want) == [(25, 200, 700, 0), (25, 200, 1200, 0),
                              (25, 700, 1200, 0), (26, 1699, 2199, 0)]
    # a 64-bit set of left symbols would drop the pairs of V: the text tells
    # one from the other
    low = H.oracle_build_index(tis, nc)
    low.bwt = np.where(low.bwt < 253, low.bwt & 63, low.bwt).astype(np.uint8)
    assert astuples(H.oracle_supermax(low, 20)) == [(26, 1699, 2199, 0)]
    for gi in (upload(V, idx), upload(V, idx, 32), upload(V, idx, 64, True),
               V.Index.build(tis, nc, idx.prefixlength)):
        same(V.findsupermaximalrepeats(gi, 20).fetch(), want)
        same(V.findsupermaximalrepeats(gi, 3).fetch(),
             H.oracle_supermax(idx, 3))


# ---- f. packed reads and the pipeline on a protein index ---------------------

def test_packed_reads_on_a_protein_index(V):
    """reads that happen to use the codes 0 .. 3 only, uploaded as 2-bit rows:
    off DNA a packed batch is turned into bytes before the search"""
    base, _ = H.load_alphabet_case("prot")
    rng = np.random.default_rng(77)
    tis = base.tis.copy()
    stretch = rng.integers(0, 4, 600).astype(np.uint8)
    keep = tis[3000:3600] == H.SEPARATOR
    tis[3000:3600] = np.where(keep, H.SEPARATOR, stretch)
    tis[9000:9300] = np.where(tis[9000:9300] == H.SEPARATOR, H.SEPARATOR,
                              A.substitute(rng, stretch[100:400], 6, 4))
    idx = H.oracle_build_index(tis, base.numofchars, base.prefixlength)
    gi = V.Index.build(tis, base.numofchars, base.prefixlength)
    assert gi.info().deepprefix == 0
    m = 24
    sym = np.concatenate([stretch[p:p + m]
                          for p in rng.integers(0, 600 - m, 200)])
    assert sym.max() <= 3
    hq = H.Queries.uniform(sym, m)
    packed = V.Queries.from_host_packed(sym, m)
    plain = gpu_queries(V, hq)
    assert packed.info().numofqueries == 200
    want = H.oracle_complete(idx, hq)
    same(V.findcompletematches(gi, plain).fetch(), want)
    same(V.findcompletematches(gi, packed).fetch(), want)
    for name, kw in A.MODES:
        want = H.oracle_querymatches(idx, hq, 8, **kw)
        same(V.findquerymatches(gi, plain, 8, **kw).fetch(), want)
        same(V.findquerymatches(gi, packed, 8, **kw).fetch(), want)


def test_pipeline_job_on_a_protein_index(V):
    """one MUM job over three batches of the golden peptides (their first 32
    residues): the batches concatenate to the oracle's list"""
    idx, q = H.load_alphabet_case("prot")
    gi = golden_index(V, "prot", "tables64")
    gi.set_queryspeedup(2)
    m = 32
    rows = [q.seq(i)[:m] for i in range(q.nq) if q.length[i] >= m]
    assert len(rows) > 150
    hq = H.Queries.uniform(np.concatenate(rows), m)
    per = (len(rows) + 2) // 3
    for mode, L, kw in ((3, 6, dict(mum=True)),
                        (2, 6, dict(mum=True, cand=True))):
        want = H.oracle_querymatches(idx, hq, L, speedup=2, **kw)
        same(run_job(V, gi, hq, mode, L, per), want)


# ---- g. drop-in: the reference's vmatch on the GPU engine --------------------

def stage(wd):
    for name in ("prot_db.fna.gz", "prot_q.fna.gz"):
        with gzip.open(os.path.join(H.GOLDEN, name), "rb") as f, \
                open(os.path.join(wd, name[:-3]), "wb") as g:
            g.write(f.read())
    for name in ("prot_short.fna", "prot11.al1"):
        shutil.copy(os.path.join(H.GOLDEN, name), os.path.join(wd, name))


@needs_binaries
@pytest.mark.parametrize("case", sorted(M))
def test_vmatch_with_gpu_engine_prints_reference_output(case, tmp_path):
    wd = str(tmp_path)
    stage(wd)
    H.run_mkvtree_ref(M[case]["index"]["mkvargs"], wd)
    name = M[case]["index"]["indexname"]
    with open(os.path.join(wd, name + ".al1"), "rb") as f, \
            open(os.path.join(H.GOLDEN, M[case]["al1"]), "rb") as g:
        assert f.read() == g.read()
    for key, run in sorted(M[case]["runs"].items()):
        rc, lines, err = run_gpu_vmatch(run["args"], wd,
                                        {"VMATCH_GPU_TRACE": "1"})
        assert (rc != 0) == (run["rc"] != 0), (key, err)
        assert len(lines) == run["lines"] > 0, (case, key)
        if key.startswith("approx_"):
            # declined by the engine (NOT_COVERED): the reference's own
            # function takes the whole batch, and nothing is traced
            assert "on the GPU" not in err, (case, key, err)
        else:
            assert "on the GPU" in err, (case, key, err)
        if run["rc"] != 0:
            assert run["stderr"].split(": ", 1)[1] in err
        md5 = hashlib.md5(("\n".join(lines) + "\n").encode()).hexdigest()
        assert md5 == run["md5_lines"], (case, key)
