"""What the post-processing host entries share (vstree_amd/csrc/host_common.h),
pinned from outside: which refusal a defective layout or list meets at every
entry, with the exact code and message -- the table below was written from
the sources before the entries were put on the shared checks, and passed on
them as they were --; the edge of the bounded text buffer at every formatter;
and the header driven by a C program of its own under the sanitizers.  No
GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers as H

NC = -4                                                 # VSA_NOT_COVERED
WHO = {"select": "vsa_select", "chain": "vsa_chain_host",
       "matchcluster": "vsa_matchcluster_host",
       "erate": "vsa_eratecluster_host", "cluster": "vsa_cluster_host"}
ENTRIES = tuple(WHO)

_text = None


def micro():
    """(symbols, separator positions) of tests/golden/micro_db.fna: three
    sequences of 31, 18 and 12 symbols"""
    global _text
    if _text is None:
        tis, ssp, _ = H.fasta_text([os.path.join(H.GOLDEN, "micro_db.fna")])
        _text = (np.ascontiguousarray(tis, np.uint8),
                 np.asarray(ssp, np.uint64))
        assert len(tis) == 63 and list(ssp) == [31, 50]
    return _text


def self_records():
    """acgtacgt at 0, 15 (sequence 0), 38 (1) and 55 (2)"""
    rec = np.zeros(3, H.MATCH_DTYPE)
    rec["length"] = 8
    rec["dbstart"] = [0, 0, 15]
    rec["queryseq"] = [15, 38, 55]
    return rec


def query_records():
    """the same matches against the sequences of the index as queries"""
    rec = np.zeros(3, H.MATCH_DTYPE)
    rec["length"] = 8
    rec["dbstart"] = [0, 0, 15]
    rec["queryseq"] = [0, 1, 2]
    rec["querystart"] = [15, 6, 4]
    return rec


def layout(V, base=2, **fields):
    """the layout of micro_db.fna, self (kind 2) or against its own sequences
    as queries (1), then the fields of vsa_sinkparams set as given"""
    tis, ssp = micro()
    kw = dict(kind=base, totallength=len(tis), markpos=ssp)
    if base != 2 and not fields.pop("noarrays", False):
        kw.update(querystart=[0, 32, 51], querylength=[31, 18, 12],
                  querytotallength=63)
    lay = V.sink_params(**kw)
    for name, value in fields.items():
        assert hasattr(lay[0], name), name
        setattr(lay[0], name, value)
    return lay


def call(V, entry, lay, rec, pal=None, **params):
    """-> (0, None) or (code, message)"""
    try:
        if entry == "select":
            V.select_host(lay, rec, pal, **params)
        elif entry == "chain":
            V.chain_host(lay, rec, pal, **params)
        elif entry == "matchcluster":
            V.matchcluster_host(lay, params.get("mode", V.MATCHCLUSTER_GAP),
                                5, rec, pal)
        elif entry == "erate":
            assert pal is None
            V.matchcluster_erate_host(lay, params.get("errorrate", 5),
                                      micro()[0], rec)
        else:
            V.cluster_host(lay, 50, 50, rec, pal)
    except V.VsaError as e:
        return e.code, e.message
    return 0, None


def TR(e):
    return (NC, WHO[e] + ": lists of a six-frame translated batch "
            "(VSA_SINK_TRANSLATED) are not covered")


def SP(e):
    return (NC, WHO[e] + ": lists of vmatch -p IDX (selfpalindromic) are not "
            "covered")


def INC(e):
    return (-2, WHO[e] + ": incomplete layout")


def PAL(e):
    return (NC, WHO[e] + ": palindromic self matches are the selfpalindromic "
            "form")


def MISFIT(e, i):
    return (-2, WHO[e] + ": record %d does not fit the layout" % i)


def KIND(k):
    return (NC, "vsa_cluster_host: only self lists and lists of vmatch -p IDX "
            "are covered, not layout kind %d" % k)


def CLMISFIT(i):
    return (-2, "vsa_cluster_host: record %d does not fit the layout (a match "
            "that leaves its sequence, or a sequence number outside the 3 of "
            "the index)" % i)


OK = (0, None)
ERSELF = (NC, "vsa_eratecluster_host: matchcluster erate covers lists of an "
          "index against itself only: the second instance of a match against "
          "queries is no stretch of the index text")
ERMISFIT = (-2, "vsa_eratecluster_host: record 2 does not fit the layout (it "
            "leaves the text or holds a separator)")

# defect -> (kind of the base layout, fields set on it)
DEFECTS = {
    "none": (2, {}),
    "translated5": (2, dict(kind=5)),
    "translated6": (2, dict(kind=6)),
    "selfpalindromic": (1, dict(selfpalindromic=1, palindromic=1)),
    "totallength0": (2, dict(totallength=0)),
    "querylength": (2, dict(totalquerylength=63)),
    "nomarkpos": (2, dict(numofsequences=2, markpos=None)),
    "noqueryarrays": (1, dict(noarrays=True, numofqueries=1)),
    "numofchars1": (2, dict(numofchars=1)),
    "kind7": (2, dict(kind=7)),
    "kindminus1": (2, dict(kind=-1)),
    # several at once: the first in the order of the checks wins
    "selfpalindromic+translated+totallength0":
        (1, dict(selfpalindromic=1, kind=5, totallength=0)),
    "translated+totallength0+numofchars1":
        (2, dict(kind=6, totallength=0, numofchars=1)),
}

# (defect, entry) -> (code, message)
LAYOUTS = {
    "none": {e: OK for e in ENTRIES},
    "translated5": dict(select=TR("select"), chain=TR("chain"),
                        matchcluster=TR("matchcluster"), erate=ERSELF,
                        cluster=KIND(5)),
    "translated6": dict(select=TR("select"), chain=TR("chain"),
                        matchcluster=TR("matchcluster"), erate=ERSELF,
                        cluster=KIND(6)),
    "selfpalindromic": dict(
        select=SP("select"), chain=SP("chain"),
        matchcluster=SP("matchcluster"), erate=SP("erate"),
        cluster=(NC, "vsa_cluster_host: record 0 is a direct match, the "
                 "layout is that of vmatch -p IDX")),
    "totallength0": dict(
        select=INC("select"), chain=INC("chain"),
        matchcluster=INC("matchcluster"),
        erate=(-2, "vsa_eratecluster_host: a layout of 0 symbols, a text of "
               "63"), cluster=CLMISFIT(0)),
    "querylength": dict(select=INC("select"), chain=INC("chain"),
                        matchcluster=INC("matchcluster"), erate=ERSELF,
                        cluster=OK),
    "nomarkpos": dict(select=OK, chain=INC("chain"), matchcluster=OK,
                      erate=OK, cluster=INC("cluster")),
    "noqueryarrays": dict(
        select=(-2, "vsa_select: the layout has no query Multiseq"),
        chain=INC("chain"), matchcluster=INC("matchcluster"), erate=ERSELF,
        cluster=KIND(1)),
    "numofchars1": dict(select=INC("select"), chain=OK, matchcluster=OK,
                        erate=OK, cluster=OK),
    "kind7": dict(select=INC("select"), chain=INC("chain"),
                  matchcluster=INC("matchcluster"), erate=ERSELF,
                  cluster=KIND(7)),
    "kindminus1": dict(select=INC("select"), chain=INC("chain"),
                       matchcluster=INC("matchcluster"), erate=ERSELF,
                       cluster=KIND(-1)),
    "selfpalindromic+translated+totallength0": dict(
        select=SP("select"), chain=SP("chain"),
        matchcluster=SP("matchcluster"), erate=SP("erate"), cluster=KIND(5)),
    "translated+totallength0+numofchars1": dict(
        select=TR("select"), chain=TR("chain"),
        matchcluster=TR("matchcluster"), erate=ERSELF, cluster=KIND(6)),
}


@pytest.mark.parametrize("defect", list(DEFECTS))
@pytest.mark.parametrize("entry", ENTRIES)
def test_a_defective_layout_meets_the_refusal_it_always_met(V, entry, defect):
    kind, fields = DEFECTS[defect]
    got = call(V, entry, layout(V, kind, **fields), self_records())
    assert got == LAYOUTS[defect][entry]


def test_the_parameters_are_looked_at_before_the_layout(V):
    """chain and matchcluster: NULL, parameters, selfpalindromic, translated,
    incomplete; select: translated, incomplete, parameters"""
    rec = self_records()
    bad = layout(V, 1, selfpalindromic=1, kind=5, totallength=0)
    assert call(V, "chain", bad, rec, kind=7) == \
        (-2, "vsa_chain_host: illegal kind 7")
    assert call(V, "chain", bad, rec, thread=True) == \
        (NC, "vsa_chain_host: chain thread (closing the gaps of a chain) is "
         "not covered")
    assert call(V, "matchcluster", bad, rec, mode=7) == \
        (-2, "vsa_matchcluster_host: illegal mode 7")
    assert call(V, "erate", bad, rec, errorrate=101) == \
        (-2, "vsa_eratecluster_host: an error rate of 101 is beyond 100")
    for fields, want in ((dict(kind=5), TR("select")),
                         (dict(numofchars=1), INC("select")),
                         ({}, (-2, "vsa_select: a sort mode needs bestnumber "
                               "> 0"))):
        assert call(V, "select", layout(V, **fields), rec, sort="la") == want


def test_a_defective_list_meets_the_refusal_it_always_met(V):
    flags = np.array([0, 1, 0], np.uint8)
    # a P record of a self list
    for e in ("select", "chain", "matchcluster"):
        assert call(V, e, layout(V), self_records(), flags) == PAL(e)
    assert call(V, "cluster", layout(V), self_records(), flags) == CLMISFIT(1)
    # ... and a record that does not fit: the first of the list is reported
    both = self_records()
    both["dbstart"][0] = 60
    assert call(V, "chain", layout(V), both, flags) == MISFIT("chain", 0)
    flags = np.array([1, 0, 0], np.uint8)
    both["dbstart"] = [0, 60, 15]
    assert call(V, "chain", layout(V), both, flags) == PAL("chain")
    # a record that leaves the text, under the self layout: chain and cluster
    # place it in a sequence, erate reads the text, select and matchcluster
    # take the numbers as they are
    out = self_records()
    out["dbstart"][2] = 60
    assert call(V, "chain", layout(V), out) == MISFIT("chain", 2)
    assert call(V, "cluster", layout(V), out) == CLMISFIT(2)
    assert call(V, "erate", layout(V), out) == ERMISFIT
    assert call(V, "select", layout(V), out) == OK
    assert call(V, "matchcluster", layout(V), out) == OK
    # a record that leaves its query, a query that does not exist
    for field, value in (("querystart", 5), ("queryseq", 3)):
        out = query_records()
        assert call(V, "chain", layout(V, 1), out) == OK
        out[field][2] = value
        for e in ("select", "chain", "matchcluster"):
            assert call(V, e, layout(V, 1), out) == MISFIT(e, 2), (e, field)
    # no list at all, and a count of 2^32 - 1 (refused before a record is
    # looked at); nothing is asked for but the stats
    lay, rec = layout(V), self_records()
    for e, fn, p, noun, outputs in (
            ("chain", V.lib.vsa_chain_host,
             V._chain_params(0, 0, 0, 1.0, False), "records",
             [None] * 5 + [0, None, 0]),
            ("matchcluster", V.lib.vsa_matchcluster_host,
             V._matchcluster_params(V.MATCHCLUSTER_GAP, 5), "matches",
             [None] * 8 + [0, None, 0, None])):
        rc = fn(C.byref(lay[0]), C.byref(p), None, None, 3, *outputs)
        assert (rc, V.messagespace()) == (-1, WHO[e] + ": NULL argument")
        rc = fn(C.byref(lay[0]), C.byref(p), V._ptr(rec), None, 0xFFFFFFFF,
                *outputs)
        assert (rc, V.messagespace()) == \
            (NC, WHO[e] + ": 4294967295 %s: only fewer than 2^32 - 1 are "
             "covered" % noun)


# ---- the bounded text buffer ------------------------------------------------

def edge(V, fmt, name):
    """fmt(buffer, capacity) -> the return value: -3 with the message and
    nothing written at capacity 0, -3 at the length of the text, the text and
    its final 0 one byte above"""
    buf = np.full(4096, 0x55, np.uint8)
    n = fmt(buf, len(buf))
    assert 0 < n < len(buf) - 1 and buf[n] == 0 and (buf[n + 1:] == 0x55).all()
    text = buf[:n].tobytes()
    assert b"\0" not in text and b"\x55" not in text
    for cap in (0, 1, n - 1, n):
        buf[:] = 0x55
        assert fmt(buf, cap) == -3
        assert V.messagespace() == "%s: %d bytes do not fit a buffer of %d" \
            % (name, n + 1, cap)
        assert (buf[cap:] == 0x55).all()
        # what fits in front of the first line that does not is written
        assert buf[:cap].tobytes() in (text[:k] + b"\x55" * (cap - k)
                                       for k in range(cap + 1))
        if cap == 0:
            assert (buf == 0x55).all()
    buf[:] = 0x55
    assert fmt(buf, n + 1) == n
    assert buf[:n + 1].tobytes() == text + b"\0" and (buf[n + 1:] == 0x55).all()
    return text


def test_every_formatter_reports_a_buffer_that_is_too_small(V):
    tis, ssp = micro()
    rec = self_records()
    sink = V.Sink(kind=V.SINK_SELF, totallength=len(tis), markpos=ssp)
    sink.setdigits()
    lines = sink.format(rec).splitlines(True)
    assert len(lines) == 3
    # two chains: records 0 and 2, record 1
    number = np.array([0, 1], np.uint64)
    score = np.array([16, -8], np.int64)
    start = np.array([0, 2, 3], np.uint64)
    members = rec[[0, 2, 1]]

    def chains(buf, cap):
        return V.lib.vsa_chain_format_host(
            sink._h, 0, 2, V._ptr(number), V._ptr(score), V._ptr(start),
            V._ptr(members), V._ptr(buf), cap)
    assert edge(V, chains, "vsa_chain_format") == \
        b"# chain 0: length 2 score 16\n" + lines[0] + lines[2] + \
        b"# chain 1: length 1 score -8\n" + lines[1]
    # the list of a clustering: the instance at 15 begins 7 symbols behind
    # the end of the one at 0, so the three matches are one cluster
    p = V._matchcluster_params(V.MATCHCLUSTER_GAP, 7)
    lay = layout(V)

    def clustering(buf, cap):
        written = C.c_int64(0)
        rc = V.lib.vsa_matchcluster_host(
            C.byref(lay[0]), C.byref(p), V._ptr(rec), None, 3, None, None,
            None, None, None, None, None, None, 0, V._ptr(buf), cap,
            C.byref(written))
        return written.value if rc == 0 else rc
    assert edge(V, clustering, "vsa_matchcluster_format") == \
        b"# cluster 3 matches\n# create cluster 0 of size 3\n"
    # the file of one cluster: its members and its edges
    member = np.array([0, 2, 1], np.uint64)
    m0 = np.array([0, 0], np.uint32)
    m1 = np.array([1, 2], np.uint32)
    value = np.array([0, 7], np.uint64)

    def cluster_file(buf, cap):
        return V.lib.vsa_matchcluster_format_host(
            sink._h, V.MATCHCLUSTER_GAP, V._ptr(member), V._ptr(members), 3,
            V._ptr(m0), V._ptr(m1), V._ptr(value), 2, V._ptr(buf), cap)
    assert edge(V, cluster_file, "vsa_matchcluster_format_cluster") == \
        b"# id 0\n" + lines[0] + b"# id 2\n" + lines[2] + b"# id 1\n" + \
        lines[1] + b"# linked 0 and 1 with gapsize 0\n" \
        b"# linked 0 and 2 with gapsize 7\n"


# ---- the header under the sanitizers ----------------------------------------

def test_shared_host_code_under_the_sanitizers_as_a_program_of_its_own(
        tmp_path):
    """scripts/host_common_check.c with the host files of chaining, match
    clustering and selection, built with -fsanitize=address,undefined: the
    message buffer, the text buffer at its edges, the layout view over every
    defect of the table above, one micro list through vsa_chain_host and
    vsa_matchcluster_host; no Python and no GPU in the process"""
    exe = str(tmp_path / "host_common_check")
    csrc = os.path.join(H.ROOT, "vstree_amd", "csrc")
    subprocess.check_call(
        ["gcc", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-Wall", "-Wextra",
         "-I" + os.path.join(H.ROOT, "include"), "-I" + csrc,
         os.path.join(H.ROOT, "scripts", "host_common_check.c")] +
        [os.path.join(csrc, f) for f in (
            "chain_host.c", "matchcluster_host.c", "cluster_host.c",
            "select_host.c", "match_sink.c")] + ["-o", exe, "-lm"])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stdout.decode() + p.stderr.decode()
    assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr
    assert p.stdout.decode().splitlines()[-1] == "host_common_check: ok"
