"""vsa_multi_pipeline_* with replicas on device 0: ragged batches whose count
is no multiple of the replicas, vsa_multi_pipeline_finish before the last
batch was taken, and candidate rows that grow in every replica.  Expected
lists: the CPU oracle over the reads of the whole job (pipeline_cases.py)."""
import numpy as np
import pytest

import pipeline_cases as PC
from test_gpu_multi import MG  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

SEAM = "VSA_PIPELINE_ROW_SLACK"


def replicas(MG, world):
    i = PC.INDEX.as_width(64)
    m = MG.Multi.from_tables(i.n, i.prefixlength, i.numofchars, i.tis, i.suf,
                             i.lcp, i.llv, i.bck, i.bwt,
                             devices=[0] * world)
    m.set_queryspeedup(2)
    return m


def finish(p, world):
    """-> (the MUMs of the job: the lists of the ranges in order, stats)"""
    lists, st = p.finish()
    for r, l in enumerate(lists):
        part = (l["dbstart"].astype(object) * world) // (PC.INDEX.n + 1)
        assert all(x == r for x in part)
    return PC.joined(lists), st


@pytest.mark.parametrize("world", [2, 3])
def test_ragged_batches_dealt_out_to_replicas(V, MG, monkeypatch, world):
    monkeypatch.delenv(SEAM, raising=False)
    m = replicas(MG, world)
    # (10 batches for three replicas, 11 for two)
    sizes = PC.RAGGED if len(PC.RAGGED) % world else PC.RAGGED + (3,)
    assert len(sizes) % world != 0
    nq = sum(sizes)
    for name in ("m33", "m100"):
        reads, ql, L = PC.READS[name], PC.length_of(name), \
            PC.searchlength(name)
        for mode in (PC.MUMCAND, PC.MEM, PC.MUM):
            want = PC.expected(name, mode, 0, nq)
            p = MG.MultiPipeline(m, mode, L, ql, PC.PER, maxspecial=PC.PER)
            lists = PC.run_job(p, reads, sizes)
            if mode == PC.MUM:
                assert all(len(l) == 0 for l in lists)
                got, st = finish(p, world)
                assert st.candidates == len(PC.expected(name, PC.MUMCAND, 0,
                                                        nq))
            else:
                assert [len(l) for l in lists] == PC.batch_counts(want, sizes)
                got = PC.joined(lists)
            assert np.array_equal(got, want), (name, mode)
            p.close()
    m.close()


@pytest.mark.parametrize("world", [2, 3])
def test_finish_before_the_last_batch_is_taken_loses_nothing(V, MG,
                                                             monkeypatch,
                                                             world):
    """world + 1 batches, all taken but the last: every replica but the one
    of the last batch could hand its rows over.  The call is refused before
    anything is touched; after the last batch is taken the job finishes with
    the list of ALL its batches."""
    monkeypatch.delenv(SEAM, raising=False)
    m = replicas(MG, world)
    name, per = "m48", 120
    reads, L = PC.READS[name], PC.searchlength(name)
    sizes = [per] * world + [per - 1]
    nq = sum(sizes)
    want = PC.expected(name, PC.MUM, 0, nq)
    p = MG.MultiPipeline(m, PC.MUM, L, 48, per)
    first = 0
    for n in sizes:
        assert PC.offer(p, reads[first:first + n], n)
        first += n
    for _ in range(world):
        assert p.next()[0] == 0
    with pytest.raises(V.VsaError) as e:
        p.finish()
    assert (e.value.code, e.value.message) == (
        -1, "vsa_multi_pipeline_finish: batches are still outstanding")
    assert len(PC.drain(p)) == 1
    got, st = finish(p, world)
    assert np.array_equal(got, want)
    assert st.candidates == len(PC.expected(name, PC.MUMCAND, 0, nq))
    # the next job of the handle: numbered from 0, dealt out from replica 0
    lists = PC.run_job(p, reads[nq:], [per, 7])
    assert all(len(l) == 0 for l in lists)
    got, st = finish(p, world)
    assert np.array_equal(got, PC.expected(name, PC.MUM, nq, per + 7))
    p.close()
    m.close()


@pytest.mark.parametrize("slack", [None, 1], ids=["unset", "1"])
def test_candidate_rows_grow_in_every_replica(V, MG, monkeypatch, slack):
    monkeypatch.delenv(SEAM, raising=False)
    if slack is not None:
        monkeypatch.setenv(SEAM, str(slack))
    world = 2
    m = replicas(MG, world)
    name, per = "m48", 100
    reads, L = PC.READS[name], PC.searchlength(name)
    sizes = [per] * 7 + [per - 1]      # four batches per replica
    nq = sum(sizes)
    cand = PC.expected(name, PC.MUMCAND, 0, nq)
    assert min(PC.batch_counts(cand, sizes)) > 1
    p = MG.MultiPipeline(m, PC.MUM, L, 48, per)
    assert all(len(l) == 0 for l in PC.run_job(p, reads, sizes))
    got, st = finish(p, world)
    assert np.array_equal(got, PC.expected(name, PC.MUM, 0, nq))
    assert st.candidates == len(cand)
    p.close()
    m.close()
