"""vsa_pipeline_* where the batches of a job differ: ragged sizes in reused
slots, lists held across later batches, match and candidate buffers that grow
under live data, several jobs on one handle, failed jobs and refused calls.

Every expected list is the CPU oracle's over the reads of the whole job as
one batch (pipeline_cases.py); the comparison is np.array_equal, order
included."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import pipeline_cases as PC

pytestmark = pytest.mark.gpu

SEAM = "VSA_PIPELINE_ROW_SLACK"
_index = []


def gpu_index(V):
    if not _index:
        i = PC.INDEX
        gi = V.Index.from_tables(i.n, i.prefixlength, i.numofchars, i.tis,
                                 i.suf, i.lcp, i.llv, i.bck, i.bwt)
        gi.set_queryspeedup(2)
        _index.append(gi)
    return _index[0]


def check_batches(lists, sizes, want, mode):
    """the lists of the batches against the job's list"""
    assert len(lists) == len(sizes)
    if mode == PC.MUM:
        assert all(len(l) == 0 for l in lists)
        return
    assert [len(l) for l in lists] == PC.batch_counts(want, sizes)
    assert np.array_equal(PC.joined(lists), want)


def refused(V, call, code, message):
    with pytest.raises(V.VsaError) as e:
        call()
    assert (e.value.code, e.value.message) == (code, message)


# ---- 1. ragged sizes, slots reused by batches of other sizes ----------------

@pytest.mark.parametrize("packed", [False, True], ids=["bytes", "packed"])
@pytest.mark.parametrize("name", PC.RICH)
def test_ragged_batches_in_reused_slots(V, monkeypatch, name, packed):
    """A short batch comes into the slot a full one left: behind its nq * W
    words + 32 bytes lie the rows of the full batch, the last of which name
    that batch's side list; behind its nspecial * m bytes lies that side
    list; the device bytes are those of the batch before (MEM remakes them).
    An empty batch delivers an empty list in its place."""
    monkeypatch.delenv(SEAM, raising=False)
    gi = gpu_index(V)
    reads, m, L = PC.READS[name], PC.length_of(name), PC.searchlength(name)
    for sizes in (PC.RAGGED, PC.STRICT):
        nq = sum(sizes)
        most = max(int(PC.wildcard_reads(reads[a:a + n]).sum())
                   for a, n in zip(PC.starts(sizes), sizes))
        assert most >= PC.NWILDLAST
        for maxspecial in ((PC.PER, most) if packed else (None,)):
            for mode in PC.MODES:
                want = PC.expected(name, mode, 0, nq)
                p = V.Pipeline(gi, mode, L, m, PC.PER, packed=packed,
                               maxspecial=maxspecial)
                lists = PC.run_job(p, reads, sizes)
                check_batches(lists, sizes, want, mode)
                if mode == PC.MUM:
                    got, st = p.finish()
                    assert np.array_equal(got, want), (sizes, maxspecial)
                    assert st.candidates == len(PC.expected(name, PC.MUMCAND,
                                                            0, nq))
                p.close()


# ---- 2. a held list survives what does not need its slot -------------------

@pytest.mark.parametrize("packed", [False, True], ids=["bytes", "packed"])
def test_a_held_list_survives_later_batches(V, monkeypatch, packed):
    monkeypatch.delenv(SEAM, raising=False)
    gi = gpu_index(V)
    name, per = "m100", 100
    reads, m, L = PC.READS[name], PC.length_of(name), PC.searchlength(name)
    sizes = [per] * 6
    want = PC.per_batch(PC.expected(name, PC.MEM, 0, sum(sizes)), sizes)
    assert all(len(w) > 0 for w in want)
    p = V.Pipeline(gi, PC.MEM, L, m, per, packed=packed)

    def submit(b):
        assert PC.offer(p, reads[b * per:(b + 1) * per], per)

    submit(0)
    rc, held = p.next(copy=False)
    assert rc == 0
    snapshot = held.copy()
    assert np.array_equal(snapshot, want[0])
    # two slots are free: batches 1 and 2 go there and complete
    submit(1)
    submit(2)
    for b in (1, 2):
        rc, got = p.next()
        assert rc == 0 and np.array_equal(got, want[b])
    assert np.array_equal(held, snapshot)
    del held
    # batches 3 and 4 fill the two free slots; the third buffer can only be
    # the slot of batch 2, the list delivered last: it is taken
    submit(3)
    submit(4)
    submit(5)
    assert not PC.offer(p, reads[:per], per)
    for b in (3, 4, 5):
        rc, got = p.next()
        assert rc == 0 and np.array_equal(got, want[b])
    assert p.next()[0] == 1
    p.close()


# ---- 3. the match buffer of a slot grows under a held list ------------------

def test_match_buffers_grow_while_a_list_is_held(V, monkeypatch):
    monkeypatch.delenv(SEAM, raising=False)
    gi = gpu_index(V)
    per, L, few = PC.DENSE_PER, PC.DENSE_L, 2
    dense = PC.READS["dense"]
    reads = np.concatenate((PC.READS["m48"][:few], dense[:6 * per]))
    assert reads.shape[1] == 48
    sizes = [few] + [per] * 6
    at = PC.starts(sizes)
    want = PC.per_batch(PC.oracle(reads, PC.MEM, L), sizes)
    # the few matches of the first batch fit what a slot holds after open,
    # no dense batch does: every slot frees its buffer and takes a bigger
    # one, slots 1 and 2 while the list of slot 0 is held
    assert 0 < len(want[0]) <= PC.slot_capacity(per)
    assert all(len(w) > PC.slot_capacity(per) > 2 * per for w in want[1:])
    for packed in (False, True):
        p = V.Pipeline(gi, PC.MEM, L, 48, per, packed=packed)
        assert PC.offer(p, reads[:few], few)
        rc, held = p.next(copy=False)
        assert rc == 0
        snapshot = held.copy()
        assert np.array_equal(snapshot, want[0])
        for b in (1, 2):
            assert PC.offer(p, reads[at[b]:at[b] + per], per)
        for b in (1, 2):
            rc, got = p.next()
            assert rc == 0 and np.array_equal(got, want[b]), b
        assert np.array_equal(held, snapshot)
        del held
        # ... and slot 0 itself, then every slot again
        rest = PC.run_job(p, reads[at[3]:], sizes[3:])
        for b, got in enumerate(rest, 3):
            assert np.array_equal(got, want[b]), b
        p.close()


# ---- 4. the candidate rows grow under live rows ----------------------------

@pytest.mark.parametrize("slack", [None, 1, 2], ids=["unset", "1", "2"])
def test_candidate_rows_grow_under_live_rows(V, monkeypatch, slack):
    """VSA_PIPELINE_ROW_SLACK = s: the buffer holds the rows so far and s
    more, so a batch with more than s candidates moves all rows of the
    batches before into a bigger one.  Unset: one allocation, the control."""
    monkeypatch.delenv(SEAM, raising=False)
    if slack is not None:
        monkeypatch.setenv(SEAM, str(slack))
    gi = gpu_index(V)
    name, per = "m48", 100
    reads, L = PC.READS[name], PC.searchlength(name)
    sizes = [per] * 7 + [per - 1]
    nq = sum(sizes)
    want = PC.expected(name, PC.MUM, 0, nq)
    cand = PC.expected(name, PC.MUMCAND, 0, nq)
    # every batch has more candidates than the slack: it grows at each
    assert min(PC.batch_counts(cand, sizes)) > 2
    for packed in (False, True):
        for compact in (False, True):
            p = V.Pipeline(gi, PC.MUM, L, 48, per, packed=packed)
            check_batches(PC.run_job(p, reads, sizes), sizes, want, PC.MUM)
            got, st = p.finish(compact=compact)
            if compact:
                got = V.expand_match16(got)
            assert np.array_equal(got, want)
            assert st.candidates == len(cand) and st.count == len(want)
            p.close()


# ---- 5. jobs ---------------------------------------------------------------

def mum_job(V, p, reads, compact):
    """a job, the short batch first -> (its MUMs as records, its stats)"""
    per, n = p.maxqueries, len(reads)
    sizes = ([n % per] if n % per else []) + [per] * (n // per)
    assert all(len(l) == 0 for l in PC.run_job(p, reads, sizes))
    got, st = p.finish(compact=compact)
    return (V.expand_match16(got) if compact else got), st


@pytest.mark.parametrize("order", ["full-compact-full", "compact-full"])
def test_every_job_of_a_mum_pipeline_is_numbered_from_zero(V, monkeypatch,
                                                           order):
    """vsa_pipeline_finish / _finish16 end a job: the reads of the next one
    count from 0 again, its list is the oracle's over its own reads.  (The
    page-locked list is kept between the jobs: a compact job sizes it in 16
    byte records, a full job reads it in 32 byte records.)"""
    monkeypatch.delenv(SEAM, raising=False)
    gi = gpu_index(V)
    reads, L = PC.READS["m100"], PC.JOBS_L
    jobs = list(zip(PC.JOBS, (False, True, False)))
    if order == "compact-full":
        jobs = [(PC.JOBS[0], True), (PC.JOBS[2], False)]
    for packed in (False, True):
        p = V.Pipeline(gi, PC.MUM, L, 100, 250, packed=packed)
        for (first, count), compact in jobs:
            own = reads[first:first + count]
            want = PC.oracle(own, PC.MUM, L)
            got, st = mum_job(V, p, own, compact)
            assert np.array_equal(got, want), (first, count, compact)
            assert st.count == len(want)
            assert st.candidates == len(PC.oracle(own, PC.MUMCAND, L))
        p.close()


@pytest.mark.parametrize("mode", [PC.COMPLETE, PC.MEM, PC.MUMCAND])
def test_numbering_continues_until_set_offset_restarts_it(V, monkeypatch,
                                                          mode):
    monkeypatch.delenv(SEAM, raising=False)
    gi = gpu_index(V)
    name = "m33"
    reads, m, L = PC.READS[name], PC.length_of(name), PC.searchlength(name)
    set_offset = lambda p, k: V._check(
        V.lib.vsa_pipeline_set_offset(p._h, int(k)))

    def shifted(first, count, k):
        want = PC.oracle(reads[first:first + count], mode, L).copy()
        want["queryseq"] += np.uint64(k)
        return want

    for packed in (False, True):
        p = V.Pipeline(gi, mode, L, m, 120, packed=packed)
        # modes 0 to 2 have no job end: drained or not, the numbers go on
        sizes = [100, 50, 120]
        a = PC.run_job(p, reads, sizes[:2])
        b = PC.run_job(p, reads[150:], sizes[2:])
        check_batches(a + b, sizes, PC.expected(name, mode, 0, 270), mode)
        set_offset(p, 0)
        got = PC.run_job(p, reads[300:], [120, 81])
        assert np.array_equal(PC.joined(got), shifted(300, 201, 0))
        p.close()
        # an offset before the first batch and between two batches that are
        # both in flight: queryseq is k + i from there
        p = V.Pipeline(gi, mode, L, m, 120, packed=packed)
        set_offset(p, 7)
        assert PC.offer(p, reads[:110], 110)
        set_offset(p, 5000)
        assert PC.offer(p, reads[400:520], 120)
        assert PC.offer(p, reads[520:523], 3)
        got = PC.drain(p)
        assert len(got) == 3
        assert np.array_equal(got[0], shifted(0, 110, 7))
        assert np.array_equal(PC.joined(got[1:]), shifted(400, 123, 5000))
        p.close()


# ---- 6. the candidate rows of a job, for a caller that filters them --------

def take_candidates(V, p):
    ptr, n, bits = C.c_void_p(), C.c_uint64(), C.c_uint32()
    V._check(V.lib.vsa_pipeline_take_candidates(p._h, C.byref(ptr),
                                                C.byref(n), C.byref(bits)))
    rows = np.zeros((n.value, 2), np.uint64)
    if n.value:
        V.device_download(rows, ptr.value, 0)
    return rows, bits.value


def test_take_candidates_hands_the_rows_of_the_job_over(V, monkeypatch):
    monkeypatch.delenv(SEAM, raising=False)
    gi = gpu_index(V)
    name = "m100"
    reads, m, L = PC.READS[name], PC.length_of(name), PC.searchlength(name)
    sizes = [150, 1, 149, 77]
    want = H.sorted_matches(PC.expected(name, PC.MUMCAND, 0, sum(sizes)))
    for packed in (False, True):
        p = V.Pipeline(gi, PC.MUM, L, m, 150, packed=packed)
        PC.run_job(p, reads, sizes)
        rows, bits = take_candidates(V, p)
        assert bits == m.bit_length()
        got = np.zeros(len(rows), H.MATCH_DTYPE)
        low = np.uint64((1 << bits) - 1)
        got["dbstart"] = rows[:, 0] >> np.uint64(bits)
        got["length"] = low - (rows[:, 0] & low)
        got["queryseq"] = rows[:, 1] >> np.uint64(16)
        got["querystart"] = rows[:, 1] & np.uint64(0xFFFF)
        assert np.array_equal(H.sorted_matches(got), want)
        # the job is over: nothing is left, and the handle takes the next
        # one (its caller numbers the reads)
        rows, _ = take_candidates(V, p)
        assert len(rows) == 0
        V._check(V.lib.vsa_pipeline_set_offset(p._h, 0))
        PC.run_job(p, reads[400:], [150, 20])
        got, st = p.finish()
        assert np.array_equal(got, PC.expected(name, PC.MUM, 400, 170))
        p.close()


# ---- 7. failure and misuse --------------------------------------------------

def test_a_failed_mum_job_has_no_list_and_the_next_job_is_clean(V,
                                                                monkeypatch):
    monkeypatch.delenv(SEAM, raising=False)
    gi = gpu_index(V)
    reads = PC.READS["m48"]
    short = "searchlength=%d must be >= %d=prefixlen" % (PC.PL - 1, PC.PL)
    for packed in (False, True):
        p = V.Pipeline(gi, PC.MUM, PC.PL - 1, 48, 64, packed=packed)
        for b in range(2):
            assert PC.offer(p, reads[b * 64:(b + 1) * 64], 64)
        for b in range(2):
            rc, got = p.next()
            assert (rc, V.messagespace(), len(got)) == (-2, short, 0)
        refused(V, p.finish, -2,
                "vsa_pipeline_finish: a batch of the job failed: " + short)
        got, st = p.finish()
        assert len(got) == 0 and st.count == 0 and st.candidates == 0
        # the handle is as it was: the next batch is answered the same way
        assert PC.offer(p, reads[:64], 64)
        assert p.next()[0] == -2 and V.messagespace() == short
        refused(V, lambda: p.finish(compact=True), -2,
                "vsa_pipeline_finish: a batch of the job failed: " + short)
        p.close()


def test_finish_with_a_batch_outstanding_is_refused_and_changes_nothing(
        V, monkeypatch):
    monkeypatch.delenv(SEAM, raising=False)
    gi = gpu_index(V)
    name = "m48"
    reads, L = PC.READS[name], PC.searchlength(name)
    sizes = [64, 64, 30]
    want = PC.expected(name, PC.MUM, 0, sum(sizes))
    for packed in (False, True):
        p = V.Pipeline(gi, PC.MUM, L, 48, 64, packed=packed)
        first = 0
        for n in sizes:
            assert PC.offer(p, reads[first:first + n], n)
            first += n
        for taken in range(len(sizes)):
            refused(V, p.finish, -1,
                    "vsa_pipeline_finish: batches are still outstanding")
            refused(V, lambda: take_candidates(V, p), -1,
                    "vsa_pipeline_take_candidates: batches are still "
                    "outstanding")
            assert p.next()[0] == 0
        got, st = p.finish()
        assert np.array_equal(got, want)
        p.close()


def test_refused_calls_leave_the_pipeline_as_it_was(V, monkeypatch):
    monkeypatch.delenv(SEAM, raising=False)
    gi = gpu_index(V)
    name = "m32"
    reads, m, L = PC.READS[name], PC.length_of(name), PC.searchlength(name)
    bad = "vsa_pipeline_open: bad argument"
    refused(V, lambda: V.Pipeline(gi, 4, L, m, 10), -1, bad)
    refused(V, lambda: V.Pipeline(gi, 1, L, 0, 10), -1, bad)
    refused(V, lambda: V.Pipeline(gi, 1, L, m, 0), -1, bad)
    refused(V, lambda: V.Pipeline(gi, 4, L, m, 10, packed=True), -1, bad)
    refused(V, lambda: V.Pipeline(gi, 3, L, 0xFFFF, 10), -2,
            "vsa_pipeline_open: reads of 65535 symbols are too long for the "
            "-mum pipeline")
    want = PC.expected(name, PC.MUMCAND, 0, 150)
    # a bytes pipeline
    p = V.Pipeline(gi, PC.MUMCAND, L, m, 100)
    nobuffer = ("vsa_pipeline_submit: no buffer handed out "
                "(vsa_pipeline_hostbuffer first)")
    refused(V, lambda: p.submit(10), -1, nobuffer)
    refused(V, p.hostrows, -1,
            "vsa_pipeline_hostrows: bad argument (a packed pipeline?)")
    refused(V, p.finish, -1,
            "vsa_pipeline_finish: bad argument (a -mum pipeline?)")
    refused(V, lambda: take_candidates(V, p), -1,
            "vsa_pipeline_take_candidates: bad argument (a -mum pipeline?)")
    buf = p.hostbuffer()
    buf[:100 * m] = reads[:100].ravel()
    refused(V, lambda: p.submit(101), -1, "vsa_pipeline_submit: bad argument")
    # the buffer is still handed out, the numbering has not moved
    p.submit(100)
    refused(V, lambda: p.submit(1), -1, nobuffer)
    assert PC.offer(p, reads[100:150], 50)
    lists = PC.drain(p)
    assert len(lists) == 2
    assert np.array_equal(PC.joined(lists), want)
    p.close()
    # a packed pipeline
    p = V.Pipeline(gi, PC.MUMCAND, L, m, 100, packed=True, maxspecial=2)
    refused(V, lambda: p.submit(10), -1,
            "vsa_pipeline_submit: bad argument (a packed pipeline takes "
            "vsa_pipeline_submit_packed)")
    packed_submit = lambda nq, ns: V._check(
        V.lib.vsa_pipeline_submit_packed(p._h, nq, ns))
    refused(V, lambda: packed_submit(10, 0), -1, nobuffer)
    rows, special = p.hostrows()
    plain = np.flatnonzero(~PC.wildcard_reads(reads))[:100]
    ns = C.c_uint64(0)
    block = np.ascontiguousarray(reads[plain])
    V._check(V.lib.vsa_pack_reads(V._ptr(block), 100, m, m, V._ptr(rows),
                                  V._ptr(special), 2, C.byref(ns)))
    assert ns.value == 0
    refused(V, lambda: packed_submit(100, 3), -1,
            "vsa_pipeline_submit_packed: bad argument")
    refused(V, lambda: packed_submit(101, 0), -1,
            "vsa_pipeline_submit: bad argument")
    packed_submit(100, 0)
    rc, got = p.next()
    assert rc == 0 and np.array_equal(
        got, PC.oracle(reads[plain], PC.MUMCAND, L))
    p.close()
