"""Approximate complete matches on the GPU at the structural edges of its
kernels: 64-bit word borders of the Myers columns (ApmColumn<W>, W = 1 .. 8),
the row blocks of the banded alignment, the first and last symbols of the
text and of every sequence, 64 piece hits of one read, the three forms of
the plan, the last read of the buffer, reads beyond 512 symbols.  The cases
are those of approx_cases.py; test_approx_model_host.py holds the same
oracle lists against the same plain model on the CPU.

Every list must be the oracle's, order included, and per read the model's
set.  Every case runs on an index built on the GPU and on one uploaded from
the CPU builder's tables, each on 32-bit and (VSA_FORCE_WIDE=1) 64-bit
device tables; as bytes and, where the reads have one length, packed;
thresholds up to 3 through the banded alignment and (VSA_APM_SCAN=1) through
the region scan.  All values are integers: equal or wrong."""
import os

import numpy as np
import pytest

import approx_cases as AC
import approx_model as A
import helpers as H

pytestmark = pytest.mark.gpu


class env:
    """a switch the library reads from the environment, set for a while"""

    def __init__(self, name, on):
        self.name, self.on = name, on

    def __enter__(self):
        self.before = os.environ.get(self.name)
        if self.on:
            os.environ[self.name] = "1"
        else:
            os.environ.pop(self.name, None)

    def __exit__(self, *exc):
        if self.before is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.before


_gpu = {}


def indexes(V, tis):
    """[(label, index)]: built on the GPU | from the CPU builder's tables, on
    32-bit | 64-bit device tables (the library reads VSA_FORCE_WIDE when an
    index is made)"""
    key = tis.tobytes()
    if key not in _gpu:
        host, made = AC.host_index(tis), []
        for wide in (False, True):
            with env("VSA_FORCE_WIDE", wide):
                built = V.Index.build(tis, 4, 0)
                tables = V.Index.from_tables(host.n, host.prefixlength, 4,
                                             host.tis, host.suf, host.lcp,
                                             host.llv, host.bck, host.bwt)
            for how, gi in (("built", built), ("tables", tables)):
                info = gi.info()
                assert info.device_integersize == (64 if wide else 32)
                assert info.prefixlength == host.prefixlength
                made.append(("%s/%s" % (how, "wide" if wide else "narrow"),
                             gi))
        _gpu[key] = made
    return _gpu[key]


def run_case(V, case):
    """every form of a case against the oracle's list and the model's set;
    -> (the oracle's list, the statistics of the runs {form: Stats})"""
    want, model = AC.expected(case)
    assert np.array_equal(A.as_set(want), model), case.name
    hq = case.queries()
    forms = [("bytes", V.Queries.from_host(hq.symbols, hq.start, hq.length))]
    if case.uniform:
        forms.append(("packed", V.Queries.from_host_packed(
            hq.symbols, len(case.reads[0]))))
    inband = case.doedist and int(case.thresholds().max()) <= 3
    stats = {}
    for iname, gi in indexes(V, case.text):
        for qname, gq in forms:
            for scan in ((False, True) if inband else (False,)):
                with env("VSA_APM_SCAN", scan):
                    res = V.findapproxcompletematches(
                        gi, gq, case.doedist, case.k, case.percent)
                got, st = res.fetch(), res.stats()
                form = (case.name, iname, qname, "scan" if scan else "default")
                assert len(got) == len(want), form
                assert np.array_equal(got, want), form
                assert np.array_equal(A.as_set(got), model), form
                assert st.count == len(want), form
                # the banded alignment counts its start positions; the
                # region scan has none
                assert (st.kernel_searches > 0) == (inband and not scan), form
                stats[form[1:]] = st
    return want, stats


@pytest.mark.parametrize("name", sorted(AC.GROUPS))
def test_border_reads_of_every_length(V, name):
    """reads cut flush to and one symbol off both ends of every sequence,
    with 0, 1 and K edit operations, some on the first and last read symbol:
    the clamps of the regions at 0 and n - 1, the band's text window at the
    end of the text, the loads into the padding on both sides, separators
    next to the first and last row or column.  Lengths 64 w - 1, 64 w and
    64 w + 1 (w = 1 .. 8; 512 = 64 VSA_APM_MAXWORDS) and, for the band, 8 t - 1,
    8 t, 8 t + 1.  band_*: K = 1, 2, 3 through k_apm_banded and, forced,
    through k_apm_verify_edist<W> / k_apm_longest<W>; scan_*: K = 4, 5;
    hamming_*: k_apm_verify_hamming.  W = ceil(m / 64): 63, 64 -> 1; 65 .. 128
    -> 2; 129 .. 192 -> 3; 193 .. 256 -> 4; 257 .. 320 -> 5; 321 .. 384 -> 6;
    385 .. 448 -> 7; 449 .. 512 -> 8."""
    seen = set()
    for case in AC.group(name):
        want, _ = run_case(V, case)
        AC.check_exercised(case, want)
        seen.add(case.words)
    if name.startswith(("band", "scan")):
        assert seen == {"band_short": {1, 2, 3}, "band_mid": {3, 4, 5, 6},
                        "band_long": {6, 7, 8}, "scan_short": {1, 2, 3, 4, 5},
                        "scan_long": {5, 6, 7, 8}}[name]


def test_short_reads_in_batches_whose_longest_read_fixes_the_words(V):
    """mixed lengths: W = 8 (longest read 512) and W = 6 (longest 384) for
    every read of the batch, the columns of the shorter ones end in an
    earlier word; 1 percent of 127 .. 384 symbols: thresholds 1, 2, 3 in one
    batch under the band of K = 3"""
    seen = set()
    for case in AC.mixed_cases():
        want, _ = run_case(V, case)
        AC.check_exercised(case, want)
        seen.add(case.words)
        answered = set(int(q) for q in want["queryseq"])
        assert answered == set(range(len(case.reads))), case.name
    assert seen == {6, 8}


@pytest.mark.parametrize("kind", ["band", "hamming"])
def test_the_three_forms_of_the_plan_answer_alike(V, kind):
    """the same reads in a batch of one length (planned through its first
    read), among 4096 reads of several lengths (thresholds and piece lengths
    uploaded per read) and among 4097 (per-length tables, filled on the
    device): every read answers as in the small batch"""
    small = AC.mixed_case(kind, 129, 2)
    base, _ = run_case(V, small)
    period = len(small.reads)
    for m in (63, 129):
        # W = 1 and W = 3 under VSA_APM_SCAN=1
        run_case(V, AC.uniform_case(kind, m))
    for case in AC.plan_cases(kind):
        want, _ = run_case(V, case)
        for q in (0, period - 1, period, len(case.reads) - 1):
            mine = want[want["queryseq"] == q]
            theirs = base[base["queryseq"] == q % period]
            assert len(mine) > 0
            for f in ("length", "dbstart", "querystart"):
                assert np.array_equal(mine[f], theirs[f]), (case.name, q, f)
    assert len(case.reads) == AC.TABLE_READS + 1


@pytest.mark.parametrize("kind", ["band", "hamming"])
@pytest.mark.parametrize("target", [63, 64, 65, 200])
def test_one_read_with_about_64_piece_hits(V, kind, target):
    """VSA_APM_SEGMAX = 64 hits of one read: up to there the hits are sorted
    inside the reads, beyond the batch takes the radix sort"""
    case = AC.hits_case(kind, target)
    assert case.hits[0] == target
    want, stats = run_case(V, case)
    for form, st in stats.items():
        assert st.candidates == case.hits[1], (form, st.candidates, case.hits)
    assert ((want["queryseq"] == 1) &
            (want["querystart"] == 0)).sum() == target // 2


@pytest.mark.parametrize("m", [65, 63])
@pytest.mark.parametrize("packed", [False, True])
def test_the_last_read_of_the_buffer(V, m, packed):
    """m % 8 = 1 and 7: the 8-byte pattern load of the band's last row block
    reaches behind the read, here behind the buffer"""
    case = AC.last_read_case(m, packed)
    want, _ = run_case(V, case)
    assert (want["queryseq"] == len(case.reads) - 1).any()


def test_a_read_of_513_symbols_is_declined_with_its_batch(V):
    """512 = 64 VSA_APM_MAXWORDS symbols is the longest read (the border
    cases have it); one symbol more and the engine declines the batch as a
    whole -- VsaError with code NOT_COVERED naming the read, no partial list,
    alone and behind reads it could answer.  Without that read the others
    are answered as the oracle answers them."""
    tis, front, long = AC.too_long_reads()
    host = AC.host_index(tis)
    for iname, gi in indexes(V, tis):
        for doedist in (True, False):
            for number, reads in ((0, [long]), (2, front + [long])):
                hq = H.Queries.from_list(reads)
                gq = V.Queries.from_host(hq.symbols, hq.start, hq.length)
                with pytest.raises(V.VsaError) as ei:
                    V.findapproxcompletematches(gi, gq, doedist, 2)
                assert ei.value.code == V.NOT_COVERED, iname
                assert ei.value.partial is None
                assert ("query %d (length 513) is not covered" % number
                        in ei.value.message), ei.value.message
            hq = H.Queries.from_list(front)
            gq = V.Queries.from_host(hq.symbols, hq.start, hq.length)
            got = V.findapproxcompletematches(gi, gq, doedist, 2).fetch()
            want = H.oracle_approx(host, hq, doedist, 2)
            assert set(int(q) for q in want["queryseq"]) == {0, 1}
            assert np.array_equal(got, want)
