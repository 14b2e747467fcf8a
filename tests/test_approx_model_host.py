"""The plain model of approximate complete matches (approx_model.py) against
the CPU oracle on every seeded edge case (approx_cases.py), over whole texts,
and against the lists recorded from the reference (golden cases c5 and c6).
No GPU.  The GPU engine meets the same cases, the same oracle lists and the
same model sets in test_gpu_approx_edges.py."""
import numpy as np
import pytest

import approx_cases as AC
import approx_model as A
import helpers as H


def same_sets(case, want, model):
    """the oracle's list as a set per read == the model's"""
    got = A.as_set(want)
    assert len(got) == len(model), (case.name, len(got), len(model))
    assert np.array_equal(got, model), case.name


@pytest.mark.parametrize("m,k,doedist", [(63, 1, True), (64, 2, True),
                                         (65, 3, True), (97, 5, True),
                                         (65, 2, False)])
def test_all_starts_at_once_is_the_definition_at_each_start(m, k, doedist):
    """the numpy form of the model against its cell-by-cell definition: at
    every start position it reports, at the k + 2 positions on either side,
    around the separators and both ends of the text, and at seeded others"""
    tis = AC.text("short")
    reads = AC.border_reads("short", m, k, doedist)[::7]
    model = A.matches(tis, reads, doedist, k)
    assert len(model) >= len(reads)
    rng = np.random.default_rng(m)
    n = len(tis)
    edges = [0, n] + [a + L for a, L in AC.sequences(tis)]
    for q, read in enumerate(reads):
        mine = model[model["queryseq"] == q]
        starts = set(int(x) for x in rng.integers(0, n, 10))
        for p in list(mine["dbstart"]) + edges:
            starts |= set(range(int(p) - k - 2, int(p) + k + 3))
        for e in edges:
            starts |= set(range(e - m - k - 1, e - m + k + 2))
        at = A.edit_at if doedist else A.hamming_at
        want = {p: at(tis, read, p, k) for p in starts if 0 <= p < n}
        want = {p: v for p, v in want.items() if v is not None}
        got = {int(r["dbstart"]): (int(r["length"]), int(r["querystart"]))
               for r in mine if int(r["dbstart"]) in starts}
        assert got == want, (q, m, k)
        assert set(int(x) for x in mine["dbstart"]) <= starts


@pytest.mark.parametrize("name", sorted(AC.GROUPS))
def test_oracle_equals_model_on_border_reads_of_every_length(name):
    for case in AC.group(name):
        want, model = AC.expected(case)
        same_sets(case, want, model)
        AC.check_exercised(case, want)


def test_oracle_equals_model_on_mixed_batches():
    for case in AC.mixed_cases():
        want, model = AC.expected(case)
        same_sets(case, want, model)
        AC.check_exercised(case, want)


@pytest.mark.parametrize("kind", ["band", "hamming"])
def test_oracle_equals_model_on_both_sides_of_the_table_plan(kind):
    for case in AC.plan_cases(kind):
        want, model = AC.expected(case)
        same_sets(case, want, model)
    assert len(case.reads) == AC.TABLE_READS + 1


@pytest.mark.parametrize("kind", ["band", "hamming"])
@pytest.mark.parametrize("target", [63, 64, 65, 200])
def test_oracle_equals_model_around_64_piece_hits_of_a_read(kind, target):
    case = AC.hits_case(kind, target)
    assert case.hits[0] == target
    want, model = AC.expected(case)
    same_sets(case, want, model)
    # every planted copy of the marked read is a match without error
    assert ((want["queryseq"] == 1) &
            (want["querystart"] == 0)).sum() == target // 2


@pytest.mark.parametrize("m", [65, 63])
@pytest.mark.parametrize("packed", [False, True])
def test_oracle_equals_model_for_the_last_read_of_the_buffer(m, packed):
    case = AC.last_read_case(m, packed)
    want, model = AC.expected(case)
    same_sets(case, want, model)
    q = case.queries()
    last = len(case.reads) - 1
    assert int(q.start[last] + q.length[last]) == len(q.symbols)
    assert (want["queryseq"] == last).any()


def test_the_oracle_answers_reads_beyond_512_symbols():
    """(the engine declines them, test_gpu_approx_edges.py)"""
    tis, front, long = AC.too_long_reads()
    reads = front + [long]
    want = H.oracle_approx(AC.host_index(tis), H.Queries.from_list(reads),
                           True, 2)
    model = A.matches(tis, reads, True, 2)
    assert np.array_equal(A.as_set(want), model)
    assert (model["queryseq"] == 2).any()


GOLDEN = [(c, k) for c in ("c5", "c6") for k in sorted(H.manifest()[c]["runs"])
          if k.startswith("approx_")]


@pytest.mark.parametrize("case,key", GOLDEN)
def test_model_equals_the_lists_recorded_from_the_reference(case, key):
    """golden lists approx_e* / approx_h* of c5 (reads of 97 .. 153 symbols,
    the pigeonhole path of the reference) and c6 (8 .. 34 symbols, its
    esaapm / esahamming path), for the reads without a special symbol.  The
    texts hold 210 002 and 48 002 symbols: the model is asked at every start
    position the reference reports, at the 8 positions on either side and at
    400 seeded positions per read, and must report the reference's records
    there and nothing else."""
    idx, q = H.load_case(case)
    spec = key[len("approx_"):]
    doedist, k = spec[0] == "e", int(spec[1:].rstrip("pb"))
    percent = 1 if spec.endswith("p") else (2 if spec.endswith("b") else 0)
    want = H.expected(case, key)
    start = np.concatenate(([0], idx.ssp + 1)).astype(np.uint64)
    rec = np.zeros(len(want), A.MATCH_DTYPE)
    rec["length"], rec["queryseq"] = want["length"], want["queryseq"]
    rec["dbstart"] = start[want["dbseq"].astype(np.int64)] + want["dbrel"]
    rec["querystart"] = want["querystart"]
    plain = [i for i in range(q.nq) if not (q.seq(i) >= H.WILDCARD).any()]
    assert len(plain) >= q.nq - 21
    renumber = np.full(q.nq, -1, np.int64)
    renumber[plain] = np.arange(len(plain))
    rec = rec[renumber[rec["queryseq"].astype(np.int64)] >= 0]
    rec["queryseq"] = renumber[rec["queryseq"].astype(np.int64)]
    rng = np.random.default_rng(len(want))
    around = np.arange(-8, 9)
    rec = A.as_set(rec)
    lo = np.searchsorted(rec["queryseq"], np.arange(len(plain)))
    hi = np.searchsorted(rec["queryseq"], np.arange(len(plain)), side="right")
    starts = []
    for i in range(len(plain)):
        s = (rec["dbstart"][lo[i]:hi[i]].astype(np.int64)[:, None] +
             around[None, :]).ravel()
        s = np.concatenate([s, rng.integers(0, idx.n, 400)])
        starts.append(np.unique(s[(s >= 0) & (s < idx.n)]))
    model = A.matches(idx.tis, [q.seq(i) for i in plain], doedist, k, percent,
                      starts)
    assert len(rec) > 400
    assert len(model) == len(rec)
    assert np.array_equal(model, rec)
