"""Inputs of the pipeline edge tests (test_gpu_pipeline_edges.py,
test_gpu_multi_pipeline_edges.py) and the one loop that drives a job through
vsa_pipeline_* (bytes or packed) and vsa_multi_pipeline_*.

One text of 32 768 symbols over four bases: random stretches, a unit of 300
symbols planted six times with a few substitutions each (a read from it has
many MEMs), a tandem of period 3, three separators, five wildcards.  Four
"rich" read sets (m = 32, 33, 48, 100: a row that ends on a word, one that
crosses it by a symbol, the benchmark's length) sampled from the text with 0
to 2 substitutions, a tenth random, about 3 % with wildcards; one "dense" set
(m = 48) from inside the planted copies.

What a job must deliver is always the CPU oracle's list over the reads of
the whole job as ONE batch.  The conditions the tests lean on are asserted
when this module is imported, on the CPU: every expected list has at least 50
records, the dense set has batches that outgrow a slot's match buffer, the
full batches of the ragged job end in wildcard reads and the short batches
that follow them in the same slot are plain."""
import numpy as np

import helpers as H

N = 32768
UNIT = 300
COPIES = (2000, 6500, 11000, 15500, 20000, 27000)
TANDEM, TANDEMLEN = 24000, 150
SEPARATORS = (8191, 17000, 25000)
WILDCARDS = (1234, 2100, 9000, 13000, 30000)

COMPLETE, MEM, MUMCAND, MUM = 0, 1, 2, 3
MODES = (COMPLETE, MEM, MUMCAND, MUM)
SLOTS = 3                       # kSlots of pipeline.hip

# ---- the ragged job -------------------------------------------------------
# With a caller that submits whenever a buffer is to be had (run_job), batch
# i and batch i + 3 share a slot.  RAGGED is the list of the issue: the full
# batch 0 lies in slot 0, the empty batch 3 leaves everything of it where it
# was, batch 6 (2 reads) and batch 9 (1 read) come into the same slot.  STRICT
# has the short batch directly three submissions behind the full one: batch 0
# (full) -> batch 3 (2 reads) -> batch 6 (1 read), and a full batch (5) behind
# a shorter one (2).
PER = 200
RAGGED = (PER, 1, PER - 1, 0, 7, PER, 2, PER, 0, 1)
STRICT = (PER, 5, PER - 1, 2, 9, PER, 1)
NWILDLAST = 3                   # wildcard reads that end every full batch


def starts(sizes):
    return [int(x) for x in np.concatenate(([0], np.cumsum(sizes)[:-1]))]


def _forced(sizes):
    """(reads that must carry a wildcard, reads that must be plain)"""
    wild, plain = set(), set()
    for i, (a, n) in enumerate(zip(starts(sizes), sizes)):
        if n == PER:
            wild.update(range(a + n - NWILDLAST, a + n))
        elif 0 < n <= 2:
            plain.update(range(a, a + n))
    return wild, plain


def _text():
    rng = np.random.default_rng(20261020)
    t = rng.integers(0, 4, N).astype(np.uint8)
    unit = rng.integers(0, 4, UNIT).astype(np.uint8)
    for c in COPIES:
        u = unit.copy()
        for _ in range(int(rng.integers(2, 6))):
            o = int(rng.integers(0, UNIT))
            u[o] = (int(u[o]) + 1 + int(rng.integers(0, 3))) % 4
        t[c:c + UNIT] = u
    t[TANDEM:TANDEM + TANDEMLEN] = np.tile(np.array([0, 2, 1], np.uint8),
                                           TANDEMLEN // 3)
    t[list(SEPARATORS)] = H.SEPARATOR
    t[list(WILDCARDS)] = H.WILDCARD
    return t


def _sample(rng, clean, nq, m, dense=False):
    out = np.empty((nq, m), np.uint8)
    for i in range(nq):
        u = rng.random()
        if dense:
            s = COPIES[int(rng.integers(0, len(COPIES)))] + \
                int(rng.integers(0, UNIT - m + 1))
        elif u < 0.1:
            out[i] = rng.integers(0, 4, m)
            s = -1
        elif u < 0.4:
            s = COPIES[int(rng.integers(0, len(COPIES)))] + \
                int(rng.integers(-(m // 2), UNIT - m // 2))
        elif u < 0.45:
            s = TANDEM + int(rng.integers(-(m // 2), TANDEMLEN - m // 2))
        else:
            s = int(rng.integers(0, N - m + 1))
        if s >= 0:
            s = min(max(s, 0), N - m)
            r = clean[s:s + m].copy()
            for _ in range(int(rng.integers(0, 2 if dense else 3))):
                o = int(rng.integers(0, m))
                r[o] = (int(r[o]) + 1 + int(rng.integers(0, 3))) % 4
            out[i] = r
        if not dense and rng.random() < 0.03:
            for _ in range(int(rng.integers(1, 4))):
                out[i, int(rng.integers(0, m))] = H.WILDCARD
    return out


def _arrange(rng, reads):
    """the forced wildcard reads and plain reads of both ragged jobs"""
    m = reads.shape[1]
    wild, plain = set(), set()
    for sizes in (RAGGED, STRICT):
        w, p = _forced(sizes)
        wild |= w
        plain |= p
    assert not (wild & plain)
    for i in sorted(plain):
        bad = reads[i] >= 4
        reads[i, bad] = rng.integers(0, 4, int(bad.sum()))
    # a wildcard in the first symbol, in the last one, and at the word border
    for k, i in enumerate(sorted(wild)):
        reads[i, (0, m - 1, min(31, m - 1))[k % 3]] = H.WILDCARD
    return reads


TEXT = _text()
INDEX = H.oracle_build_index(TEXT, 4)
PL = INDEX.prefixlength

# name -> (number of reads, m, search length of modes 1 to 3)
SETS = {"m32": (900, 32, 12), "m33": (900, 33, 12), "m48": (900, 48, 14),
        "m100": (1200, 100, 16)}
RICH = tuple(SETS)
DENSE_L = PL + 1
DENSE_PER = 64
# the -mum jobs of one handle: (first read, reads) of set m100, a small job,
# a larger one, a yet larger one; their search length
JOBS = ((0, 100), (100, 400), (500, 700))
JOBS_L = 8


def _readsets():
    clean = TEXT.copy()
    rng = np.random.default_rng(77)
    bad = clean >= 4
    clean[bad] = rng.integers(0, 4, int(bad.sum()))
    out = {}
    for name, (nq, m, _) in SETS.items():
        out[name] = _arrange(rng, _sample(rng, clean, nq, m))
    out["dense"] = _sample(rng, clean, 8 * DENSE_PER, 48, dense=True)
    return out


READS = _readsets()


def length_of(name):
    return READS[name].shape[1]


def searchlength(name):
    return DENSE_L if name == "dense" else SETS[name][2]


def wildcard_reads(reads):
    return (reads >= 4).any(axis=1)


def oracle(reads, mode, L):
    """the list of a job whose reads are `reads` (nq x m), as one batch"""
    reads = np.ascontiguousarray(reads, np.uint8)
    q = H.Queries.uniform(reads.ravel(), reads.shape[1])
    if mode == COMPLETE:
        want = H.oracle_complete(INDEX, q)
    else:
        want = H.oracle_querymatches(INDEX, q, L, speedup=2,
                                     mum=mode in (MUMCAND, MUM),
                                     cand=mode == MUMCAND)
    # (no test compares two empty lists)
    assert len(want) >= 50, (reads.shape, mode, L, len(want))
    return want


_expected = {}


def expected(name, mode, first=0, count=None):
    """oracle(reads [first, first + count) of a set, numbered from 0)"""
    count = len(READS[name]) - first if count is None else count
    k = (name, mode, first, count)
    if k not in _expected:
        _expected[k] = oracle(READS[name][first:first + count], mode,
                              searchlength(name))
        _expected[k].setflags(write=False)
    return _expected[k]


def per_batch(want, sizes):
    """the records of a job's list batch by batch: queryseq ascends over
    the list in modes 0 to 2"""
    edges = np.concatenate(([0], np.cumsum(sizes))).astype(np.uint64)
    cut = np.searchsorted(want["queryseq"], edges)
    return [want[cut[i]:cut[i + 1]] for i in range(len(sizes))]


def batch_counts(want, sizes):
    """records per batch of any list (also one in another order)"""
    edges = np.concatenate(([0], np.cumsum(sizes)))
    return [int(((want["queryseq"] >= edges[i]) &
                 (want["queryseq"] < edges[i + 1])).sum())
            for i in range(len(sizes))]


def slot_capacity(per):
    """records the match buffer of a slot holds after vsa_pipeline_open
    (growhost of pipeline.hip: asked for 1.5 per, it takes a quarter more and
    1024)"""
    need = per + per // 2
    return need + need // 4 + 1024


# ---- the driver -----------------------------------------------------------

def offer(p, block, n):
    """the next batch into a free slot; False: all batches are in flight"""
    if not getattr(p, "packed", True):     # (a multi pipeline is packed)
        buf = p.hostbuffer()
        if buf is None:
            return False
        buf[:block.size] = block.ravel()
        p.submit(n)
        return True
    m = p.m
    return p.pack_into_slot(block.ravel() if n else np.zeros(m, np.uint8), n)


def run_job(p, reads, sizes, copy=True):
    """submits reads (nq x m) in batches of `sizes`, as early as a buffer is
    to be had, and takes every batch; -> the lists of the batches in order.
    Serves a bytes pipeline, a packed one and a multi pipeline."""
    assert sum(sizes) <= len(reads)
    out, first = [], 0
    for n in sizes:
        block = reads[first:first + n]
        while not offer(p, block, n):
            rc, got = p.next(copy=copy)
            assert rc == 0, rc
            out.append(got)
        first += n
    out += drain(p, copy)
    assert len(out) == len(sizes)
    return out


def drain(p, copy=True):
    """the lists of all batches not taken yet"""
    out = []
    while True:
        rc, got = p.next(copy=copy)
        if rc == 1:
            return out
        assert rc == 0, rc
        out.append(got)


def joined(lists):
    lists = [l for l in lists if len(l)]
    return (np.concatenate(lists) if lists
            else np.zeros(0, H.MATCH_DTYPE))


# ---- the conditions the tests lean on -------------------------------------

def _check_inputs():
    assert len(TEXT) <= 32768 and int((TEXT < 4).sum()) == \
        N - len(SEPARATORS) - len(WILDCARDS)
    for sizes in (RAGGED, STRICT):
        wild, plain = _forced(sizes)
        assert wild and plain
        nq = sum(sizes)
        for name in RICH:
            reads = READS[name]
            assert 600 <= len(reads) <= 1200 and nq <= len(reads)
            w = wildcard_reads(reads)
            assert all(w[i] for i in wild) and not any(w[i] for i in plain)
            for mode in MODES:
                want = expected(name, mode, 0, nq)
                if mode != MUM:
                    # the short batches behind a full one have something to
                    # deliver, so rows of the batch before would show
                    cnt = batch_counts(want, sizes)
                    assert all(c > 0 for c, n in zip(cnt, sizes) if n >= PER)
    # stale rows: behind the nq * W words + 32 bytes a short batch uploads,
    # the slot still holds the rows of the full batch before, the last of
    # which name entries of that batch's side list
    for name in RICH:
        m = length_of(name)
        W = (2 * m + 8 + 63) // 64
        assert 2 * W * 8 + 32 < (PER - NWILDLAST) * W * 8
    # the dense set: more than 2 matches per read over every window of 64
    # reads, and batches that outgrow what a slot starts with
    want = expected("dense", MEM)
    per_read = np.bincount(want["queryseq"].astype(np.int64),
                           minlength=len(READS["dense"]))
    windows = np.convolve(per_read, np.ones(DENSE_PER, np.int64), "valid")
    assert int(windows.min()) > 2 * DENSE_PER
    assert DENSE_L > PL
    # the jobs of one -mum handle: lists of different sizes, and a full list
    # that does not fit the page-locked room a compact one of the first job
    # asked for (pipeline_finish of pipeline.hip: c + c / 8 + 1024 records of
    # 16 bytes)
    mums = [len(oracle(READS["m100"][a:a + n], MUM, JOBS_L)) for a, n in JOBS]
    assert mums[0] < mums[1] < mums[2]
    assert mums[2] * 32 > (mums[0] + mums[0] // 8 + 1024 + 2) * 16


_check_inputs()
