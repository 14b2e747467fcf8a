"""Match coverage without a GPU: a numpy restatement of the reference's
markmatches (Vmatch/markmat.c:42-118) and nomatchsubstringsout
(Vmatch/nomatch.c:168-274) reproduces every recorded answer of the real
reference (tests/golden/coverage_*, scripts/make_golden_coverage.py) from the
recorded match lists -- the model the GPU tests compare the kernels with --
and the host formatter / masker reproduce the reference's text."""
import hashlib
import json
import os

import numpy as np
import pytest

import helpers as H

QUERY, SELF, APPROX = 0, 1, 2
DATABASE, QUERIES = 0, 1
ALLFLAGS = dict(markleft=1, markright=1, markleftifdifferentsequence=1,
                markrightifdifferentsequence=1)
KEEP = {"keepleft": "markleft", "keepright": "markright",
        "keepleftifsamesequence": "markleftifdifferentsequence",
        "keeprightifsamesequence": "markrightifdifferentsequence"}

with open(os.path.join(H.GOLDEN, "coverage_manifest.json")) as f:
    CM = json.load(f)
RUNS = [(c, k) for c in sorted(CM) for k in sorted(CM[c])]
_cexp = None


def cexpected(name):
    global _cexp
    if _cexp is None:
        _cexp = np.load(os.path.join(H.GOLDEN, "coverage_expected.npz"))
    return _cexp[name]


# --------------------------------------------------------------------------
# the model
# --------------------------------------------------------------------------

class Table:
    """the reference's marktable over a Multiseq: one bool per position, the
    separators set (initmarktable, markmat.c:15-28)"""

    def __init__(self, nbits, ssp, dblength=None, numofdbsequences=None,
                 seqoffset=0):
        self.ssp = np.asarray(ssp, np.int64)
        self.marked = np.zeros(int(nbits), bool)
        self.marked[self.ssp] = True
        self.dblength, self.numofdbsequences = dblength, numofdbsequences
        self.seqoffset = seqoffset
        self.starts = np.concatenate(([0], self.ssp + 1))
        self.ends = np.concatenate((self.ssp, [int(nbits)]))

    @property
    def hasindexedqueries(self):
        return self.dblength is not None

    def seqnum(self, pos):
        return int(np.searchsorted(self.ssp, pos, side="left"))

    def words(self):
        pad = np.zeros((len(self.marked) + 63) // 64 * 64, bool)
        pad[:len(self.marked)] = self.marked
        return np.packbits(pad, bitorder="little").view(np.uint64)

    def count(self):
        return int(self.marked.sum()) - len(self.ssp)


def model_mark(t, rec, layout, side, palindromic=False, markleft=1,
               markright=1, markleftifdifferentsequence=1,
               markrightifdifferentsequence=1):
    """markmatches for engine records (length, dbstart, queryseq,
    querystart) of the given layout, in the reference's terms"""
    markdb = side == DATABASE
    hasnoqueryfiles = layout == SELF
    for m in rec:
        length = int(m["length"])
        pos1, len1, len2 = int(m["dbstart"]), length, length
        seq1 = seq2 = pos2 = None
        if layout == SELF:
            # convertthematch, Vmatch/procfinal.c:450-475
            pos2, seq1 = int(m["queryseq"]), t.seqnum(pos1)
            seq2 = t.seqnum(pos2)
            if t.hasindexedqueries:
                seq2 -= t.numofdbsequences
                pos2 -= t.dblength + 1
        else:
            assert markleftifdifferentsequence and markrightifdifferentsequence
            if not markdb:
                assert layout == QUERY
                q = int(m["queryseq"]) - t.seqoffset
                seqlen = int(t.ends[q] - t.starts[q])
                rel = int(m["querystart"])
                if palindromic:                      # procfinal.c:152-158
                    rel = seqlen - (rel + length)
                pos2 = int(t.starts[q]) + rel
        if markleft and markdb:
            if markleftifdifferentsequence or seq1 != seq2:
                t.marked[pos1:pos1 + len1] = True
        if not markdb or hasnoqueryfiles:
            if ((not markdb or markright) and
                    (markrightifdifferentsequence or seq1 != seq2)):
                offset = (0 if markdb or not t.hasindexedqueries or
                          layout != SELF else t.dblength + 1)
                assert pos2 >= 0
                t.marked[offset + pos2:offset + pos2 + len2] = True


def model_nomatch(t, minlength, first=0, length=None):
    """nomatchsubstringsout -> rows (length, absolute start, seqnum,
    relative start) with the TRUE sequence number"""
    length = len(t.marked) - first if length is None else length
    clear = ~t.marked[first:first + length]
    d = np.diff(np.concatenate(([0], clear.astype(np.int8), [0])))
    s, e = np.flatnonzero(d == 1) + first, np.flatnonzero(d == -1) + first
    keep = e - s >= minlength
    s, e = s[keep], e[keep]
    seq = np.searchsorted(t.ssp, s, side="left")
    out = np.zeros(len(s), np.dtype([("length", "<u8"), ("start", "<u8"),
                                     ("seqnum", "<u8"), ("relstart", "<u8")]))
    out["length"], out["start"], out["seqnum"] = e - s, s, seq
    out["relstart"] = s - t.starts[seq]
    return out


def rows_as_printed(iv, absolute, posoffset):
    """what shownomatch prints for the runs, as integers"""
    if absolute:
        return np.stack([iv["start"] - np.uint64(posoffset), iv["length"]],
                        axis=1)
    if posoffset:
        return np.stack([np.zeros(len(iv), np.uint64),
                         iv["start"] - np.uint64(posoffset), iv["length"]],
                        axis=1)
    return np.stack([iv["seqnum"], iv["relstart"], iv["length"]], axis=1)


# --------------------------------------------------------------------------
# the recorded runs
# --------------------------------------------------------------------------

_alltext = {}


def all_text(case):
    """Multiseq of the index `all` of a case: database then queries"""
    if case not in _alltext:
        m = H.manifest()[case]
        files = [H._golden_fasta(f) for f in m["db"]] + \
            [H._golden_fasta(m["query"])]
        tis, ssp, perfile = H.fasta_text(files)
        ndb = sum(perfile[:len(m["db"])])
        _alltext[case] = (tis, ssp, int(ssp[ndb - 1]), ndb)
    return _alltext[case]


def query_ssp(q):
    return (np.cumsum(q.length.astype(np.int64) + 1) - 1)[:-1]


def new_table(case, e):
    """the table the reference makes for a run (initpost.c:28-74)"""
    idx, q = H.load_case(case)
    if e["index"] == "all":
        tis, ssp, dblen, ndb = all_text(case)
        return Table(len(tis), ssp, dblen, ndb)
    if e["side"] == "db" or e["engine"] == "complete":
        return Table(idx.n, idx.ssp)
    return Table(int(q.length.sum()) + q.nq - 1, query_ssp(q))


def run_layout(e):
    if e["engine"] == "query":
        return QUERY
    if e["engine"] == "complete":
        return APPROX if e["approx"] else QUERY
    return SELF


def run_flags(e):
    flags = dict(ALLFLAGS)
    if e["keep"]:
        flags[KEEP[e["keep"]]] = 0
    return flags


def recorded_records(case, e):
    """the recorded match list of a run as engine records -> list of
    (records, palindromic)"""
    idx, q = H.load_case(case)
    src = e["matches"]
    if src.startswith("expected:"):
        x = H.expected(case, src[len("expected:"):])
        m = np.stack([x[k] for k in x.dtype.names] +
                     [np.zeros(len(x), np.uint64)], axis=1)
    else:
        m = cexpected(src)
    m = m.astype(np.int64)
    layout = run_layout(e)
    if e["index"] == "all":
        tis, ssp, dblen, ndb = all_text(case)
    else:
        ssp, ndb = idx.ssp.astype(np.int64), 0
    starts = np.concatenate(([0], ssp + 1)).astype(np.int64)
    out = []
    for pal in (0, 1):
        x = m[m[:, 5] == pal]
        if pal and not len(x):
            continue
        rec = np.zeros(len(x), H.MATCH_DTYPE)
        rec["length"] = x[:, 0]
        rec["dbstart"] = starts[x[:, 1]] + x[:, 2]
        if layout == SELF:
            rec["queryseq"] = starts[x[:, 3] + ndb] + x[:, 4]
        else:
            rec["queryseq"] = x[:, 3]
            rel = x[:, 4]
            if pal:     # the engine reports positions on the reverse strand
                rel = q.length[x[:, 3]].astype(np.int64) - (rel + x[:, 0])
            rec["querystart"] = rel
        out.append((rec, bool(pal)))
    return out


def run_range(t, e):
    """(first, length, posoffset) of the reference's scan (initpost.c:156)"""
    if e["index"] == "all":
        if e["side"] == "db":
            return 0, t.dblength, 0
        return t.dblength + 1, len(t.marked) - t.dblength - 1, t.dblength + 1
    if run_layout(e) == SELF:
        # DATABASELENGTH = totallength - 0 - 1 (include/multidef.h:91): the
        # reference leaves the last position out
        return 0, len(t.marked) - 1, 0
    return 0, len(t.marked), 0


def check_run(case, key, table, V):
    """a marked table (model Table or anything with .marked) against the
    fixture of a run"""
    e = CM[case][key]
    name = "%s__%s" % (case, key)
    if e["mask"]:
        sep = np.zeros(len(table.marked), bool)
        sep[table.ssp] = True
        flags = table.marked & ~sep
        d = np.diff(np.concatenate(([0], flags.astype(np.int8), [0])))
        s, en = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
        assert np.array_equal(np.stack([s, en - s], axis=1),
                              cexpected(name + "__masked"))
        assert table.count() == e["masked"]
        assert len(table.marked) - len(table.ssp) == e["positions"]
        return
    first, length, posoffset = run_range(table, e)
    iv = model_nomatch(table, e["minlength"], first, length)
    assert np.array_equal(rows_as_printed(iv, e["absolute"], posoffset),
                          cexpected(name + "__intervals"))


@pytest.mark.parametrize("case,key", RUNS)
def test_model_reproduces_the_reference_from_the_recorded_lists(V, case, key):
    e = CM[case][key]
    t = new_table(case, e)
    side = DATABASE if e["side"] == "db" else QUERIES
    for rec, pal in recorded_records(case, e):
        model_mark(t, rec, run_layout(e), side, pal, **run_flags(e))
    check_run(case, key, t, V)


@pytest.mark.parametrize("case,key", [(c, k) for c, k in RUNS
                                      if not CM[c][k]["mask"]])
def test_formatter_reproduces_the_references_lines(V, case, key):
    e = CM[case][key]
    t = new_table(case, e)
    side = DATABASE if e["side"] == "db" else QUERIES
    for rec, pal in recorded_records(case, e):
        model_mark(t, rec, run_layout(e), side, pal, **run_flags(e))
    first, length, posoffset = run_range(t, e)
    iv = model_nomatch(t, e["minlength"], first, length)
    for absolute in (False, True):
        text = V.nomatch_format(iv, V.SHOW_ABSOLUTE if absolute else 0,
                                posoffset)
        rows = rows_as_printed(iv, absolute, posoffset)
        want = "".join(">" + " ".join(str(int(x)) for x in r) + "\n"
                       for r in rows)
        assert text.decode() == want
        if absolute == e["absolute"]:
            assert text.count(b"\n") == e["lines"]
            assert hashlib.md5(text).hexdigest() == e["md5_lines"]


def multiseq_chars(case, e):
    """the characters showmaskedseq reads: the sequences of the FASTA file,
    separators between them"""
    m = H.manifest()[case]
    name = m["db"][0] if e["side"] == "db" else m["query"]
    recs = H.read_fasta(H._golden_fasta(name))
    return np.frombuffer(b"\xff".join(s for _, s in recs), np.uint8)


@pytest.mark.parametrize("case,key", [(c, k) for c, k in RUNS
                                      if CM[c][k]["mask"]])
def test_mask_apply_reproduces_the_masked_sequences(V, case, key):
    e = CM[case][key]
    t = new_table(case, e)
    side = DATABASE if e["side"] == "db" else QUERIES
    for rec, pal in recorded_records(case, e):
        model_mark(t, rec, run_layout(e), side, pal, **run_flags(e))
    chars = multiseq_chars(case, e)
    assert len(chars) == len(t.marked)
    out, n = V.mask_apply(t.words(), chars, "x")
    assert n == e["masked"]
    assert (out == 255).sum() == len(t.ssp)
    body = out.tobytes().replace(b"\xff", b"\n") + b"\n"
    assert hashlib.md5(body).hexdigest() == e["md5_body"]
    if case == "micro" and key == "q_l3_dbmask":
        assert body.startswith(b"xxxxxxxxxxxxxnnxxxxxxxxxaccgxxx\n")


def test_mask_apply_case_conversion_and_the_star_rule(V):
    bits = np.array([0b0110111], np.uint64)
    chars = np.frombuffer(b"ac*g\xfftA", np.uint8)
    out, n = V.mask_apply(bits, chars, V.MASK_TOUPPER)
    assert out.tobytes() == b"AC*g\xffTA" and n == 4
    out, n = V.mask_apply(bits, np.frombuffer(b"AC*g\xffTa", np.uint8),
                          V.MASK_TOLOWER)
    assert out.tobytes() == b"ac*g\xffta" and n == 4
    # a marked character that is neither of the other case nor '*'
    with pytest.raises(V.VsaError) as err:
        V.mask_apply(bits, np.frombuffer(b"aC*g\xfftA", np.uint8),
                     V.MASK_TOUPPER)
    assert err.value.code == -4
    assert err.value.message == "cannot convert character C to upper case"
    with pytest.raises(V.VsaError) as err:
        V.mask_apply(bits, np.frombuffer(b"AC*g\xff1a", np.uint8),
                     V.MASK_TOLOWER)
    assert err.value.message == "cannot convert character 1 to lower case"
    # a literal mask character leaves unmarked ones and separators alone
    out, n = V.mask_apply(np.array([~np.uint64(0)]), chars, "N")
    assert out.tobytes() == b"NNNN\xffNN" and n == 6


def test_keep_keywords_and_their_error_with_query_files(V):
    assert V.coverage_options() == ALLFLAGS
    for kw, field in KEEP.items():
        want = dict(ALLFLAGS)
        want[field] = 0
        assert V.coverage_options(kw) == want
        with pytest.raises(V.VsaError) as err:
            V.coverage_options(kw, withquery=True, option="-dbnomatch")
        assert err.value.message == ('argument "%s" to option -dbnomatch not '
                                     'allowed if option -q is used' % kw)
    with pytest.raises(V.VsaError):
        V.coverage_options("keepboth")


def test_every_coverage_entry_of_the_header_has_its_mirror(V):
    import re
    text = open(os.path.join(H.ROOT, "include", "vstree_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = set(re.findall(r"\b(vsa_(?:coverage|nomatch|mask)_[a-z0-9_]+)\s*\(",
                          text)) | {"vsa_result_from_host"}
    assert len(syms) >= 16
    assert syms <= set(V.ABI_SYMBOLS)
    for s in syms:
        assert getattr(V.lib, s).argtypes is not None
    # the structures have the size the C compiler gives them
    assert V.C.sizeof(V.CoverageParams) == 9 * 4
    assert V.C.sizeof(V.CoverageStats) == 6 * 8
    assert V.COVERAGE_COOP_THRESHOLD == 1024
