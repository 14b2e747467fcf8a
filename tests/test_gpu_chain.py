"""Chaining on the GPU (vsa_chain_*): every recorded run of the real
reference through V.Chain against the manifest, and the kernels against
vsa_chain_host (tables and text identical) and the pure-Python model on
synthetic lists -- the sizes at which a problem changes its kernel, a problem
at the bound and one beyond it, many tiny problems in one call, and
hand-made lists that pin one rule each: the tie between equal priorities,
touching fragments, a start at 0, maxgap on the best candidate only,
negative scores, the truncated weight, repeated scores under Kb, a second
strand, the order the grouping's quicksort leaves, positions above 2^32."""
import numpy as np
import pytest

import helpers as H
import chain_cases as CS
import chain_model as CH

pytestmark = pytest.mark.gpu

SEQLEN = 1000
KINDS = [(CH.GLOBAL, 0), (CH.GLOBAL_GC, 0), (CH.GLOBAL_OV, 0),
         (CH.LOCAL_MAX, 0), (CH.LOCAL_THRESHOLD, 30), (CH.LOCAL_BEST, 2),
         (CH.LOCAL_PERCENT, 30)]
ARRAYS = ("problem", "number", "score", "start", "members")


def layout_of(V, nseq, seqlen=SEQLEN):
    """nseq sequences of seqlen symbols, matches of the index against
    itself -> (sink parameters, separator positions)"""
    markpos = np.arange(1, nseq, dtype=np.uint64) * np.uint64(seqlen + 1) - \
        np.uint64(1)
    kw = dict(kind=2, totallength=nseq * (seqlen + 1) - 1, markpos=markpos)
    return V.sink_params(**kw), kw


def records(seq1, rel1, seq2, rel2, length, seqlen=SEQLEN):
    n = len(np.atleast_1d(rel1))
    rec = np.zeros(n, H.MATCH_DTYPE)
    rec["length"] = length
    rec["dbstart"] = np.asarray(seq1, np.uint64) * np.uint64(seqlen + 1) + \
        np.asarray(rel1, np.uint64)
    rec["queryseq"] = np.asarray(seq2, np.uint64) * np.uint64(seqlen + 1) + \
        np.asarray(rel2, np.uint64)
    return rec


def model_of(kw, rec, **opt):
    mark = kw["markpos"].astype(np.int64)
    p1 = rec["dbstart"].astype(np.int64)
    p2 = rec["queryseq"].astype(np.int64)
    l1 = rec["length"].astype(np.int64).tolist()
    return CH.chain(l1, p1.tolist(), l1, p2.tolist(),
                    np.searchsorted(mark, p1).tolist(),
                    np.searchsorted(mark, p2).tolist(), form="rule", **opt)


def device_of(V, layout, parts, **opt):
    ch = V.Chain(layout, **opt)
    for rec, pal in parts:
        ch.add(V.Result.from_host(rec), pal)
    ch.finish()
    return ch


def same_as_host(V, ch, host, kw=None, silent=False):
    assert ch.stats().asdict() == host["stats"].asdict()
    got = ch.chains()
    for k in ARRAYS:
        assert np.array_equal(got[k], host[k]), k
    if kw is not None:
        sink = V.Sink(**kw)
        rec = ch.records()[0].fetch()
        assert ch.format(sink, silent) == V.chain_format_host(
            sink, host["number"], host["score"], host["start"], rec, silent)
    return got


def run(V, nseq, rec, model=True, seqlen=SEQLEN, **opt):
    """a self list through the device, vsa_chain_host and the model"""
    layout, kw = layout_of(V, nseq, seqlen)
    ch = device_of(V, layout, [(rec, False)], **opt)
    host = V.chain_host(layout, rec, **opt)
    got = same_as_host(V, ch, host, kw)
    res, flags = ch.records()
    assert np.array_equal(res.fetch(), rec[got["members"].astype(np.int64)])
    assert not flags.any()
    if model:
        want = model_of(kw, rec, **opt)
        assert host["stats"].asdict() == want["stats"]
        arr = CS.as_arrays(want)
        for k in ARRAYS:
            assert np.array_equal(got[k], arr[k]), k
    return ch, got


def chains_of(got):
    s = got["start"].astype(np.int64)
    return [(int(got["score"][c]), got["members"][s[c]:s[c + 1]].tolist())
            for c in range(len(got["score"]))]


# --------------------------------------------------------------------------
# the recorded runs
# --------------------------------------------------------------------------

@pytest.mark.parametrize("key", CS.keys())
def test_recorded_runs(V, key):
    r = CS.run_of(key)
    rec, flags = CS.input_of(key)
    layout = V.sink_params(**CS.layout_kwargs(r))
    assert np.array_equal(flags, np.sort(flags))     # the D pass comes first
    ch = device_of(V, layout, [(rec[flags == f], bool(f))
                               for f in sorted(set(flags.tolist()))],
                   **CS.options(r))
    got = ch.chains()
    lines = CS.lines_of(V, r, rec, flags)
    CS.check_against_manifest(key, ch.stats().asdict(), got,
                              CS.text_of(got, lines, r["silent"]))
    res, pal = ch.records()
    who = got["members"].astype(np.int64)
    assert np.array_equal(res.fetch(), rec[who])
    assert np.array_equal(pal, flags[who])
    if not flags.any():
        text = ch.format(V.Sink(**CS.layout_kwargs(r)), r["silent"])
        assert CS.md5(text) == CS.manifest()["runs"][key]["md5_text"]
    assert all(v >= 0 for v in ch.times().values())


# --------------------------------------------------------------------------
# the sizes at which a problem changes its kernel
# --------------------------------------------------------------------------

def crowded(rng, seq1, seq2, n, span, seqlen=SEQLEN):
    """n fragments of one pair with coordinates in 0 .. span: many chains,
    many ties"""
    return records(seq1, rng.integers(0, span, n), seq2,
                   rng.integers(0, span, n), rng.integers(1, 9, n), seqlen)


@pytest.mark.parametrize("kind, value", KINDS)
@pytest.mark.parametrize("maxgap", [0, 12])
def test_problems_at_the_class_boundaries(V, kind, value, maxgap):
    rng = np.random.default_rng(100 * kind + maxgap)
    sizes = [1, 2, 8, 9, 64, 65, 256, 257, 700]
    rec = np.concatenate([crowded(rng, p, p + 1, n, min(8 + 2 * n, 900))
                          for p, n in enumerate(sizes)])
    rec = rec[rng.permutation(len(rec))]
    ch, got = run(V, len(sizes) + 1, rec, kind=kind, value=value,
                  maxgap=maxgap, withinborders=True)
    st = ch.stats()
    assert (st.problems, st.single, st.small, st.wave, st.group,
            st.largest) == (9, 1, 2, 2, 4, 700)


@pytest.mark.parametrize("kind, value", [(CH.LOCAL_THRESHOLD, 25),
                                         (CH.GLOBAL_GC, 0)])
def test_a_problem_at_the_bound(V, kind, value):
    rng = np.random.default_rng(15)
    n, seqlen = V.CHAIN_MAXGROUP, 1 << 18
    rec = crowded(rng, 0, 0, n, n, seqlen)
    ch, got = run(V, 1, rec, model=False, seqlen=seqlen, kind=kind,
                  value=value, maxgap=0 if kind != CH.GLOBAL_GC else 900)
    st = ch.stats()
    assert (st.problems, st.group, st.largest) == (1, 1, n)
    assert st.chained >= st.chains > 0


def test_a_problem_beyond_the_bound_is_refused(V):
    rng = np.random.default_rng(16)
    seqlen = 1 << 17
    layout, kw = layout_of(V, 3, seqlen)
    small = crowded(rng, 0, 1, 40, 60, seqlen)
    ch = device_of(V, layout, [(small, False)], kind=CH.LOCAL_MAX,
                   withinborders=True)
    before = V.chain_host(layout, small, kind=CH.LOCAL_MAX,
                          withinborders=True)
    same_as_host(V, ch, before, kw)
    big = crowded(rng, 1, 2, V.CHAIN_MAXGROUP + 1, 1 << 16, seqlen)
    ch.add(V.Result.from_host(big))
    with pytest.raises(V.VsaError) as e:
        ch.finish()
    assert e.value.code == V.NOT_COVERED
    assert "%d fragments" % (V.CHAIN_MAXGROUP + 1) in e.value.message
    same_as_host(V, ch, before, kw)              # the state of the last finish
    # the host code takes it
    st = V.chain_host(layout, np.concatenate([small, big]),
                      kind=CH.LOCAL_MAX, withinborders=True)["stats"]
    assert st.largest == V.CHAIN_MAXGROUP + 1
    # the refused lists are gone: a smaller one on the same handle
    more = crowded(rng, 1, 2, 300, 700, seqlen)
    ch.add(V.Result.from_host(more))
    ch.finish()
    both = np.concatenate([small, more])
    got = same_as_host(V, ch, V.chain_host(layout, both, kind=CH.LOCAL_MAX,
                                           withinborders=True), kw)
    assert ch.stats().problems == 2
    assert np.array_equal(ch.records()[0].fetch(),
                          both[got["members"].astype(np.int64)])


@pytest.mark.parametrize("kind, value", [(CH.LOCAL_MAX, 0),
                                         (CH.GLOBAL_GC, 0)])
def test_fifty_thousand_tiny_problems_in_one_call(V, kind, value):
    rng = np.random.default_rng(50)
    nseq, seqlen, pairs = 250, 64, 50000
    size = rng.integers(1, 7, pairs)
    pair = np.repeat(np.arange(pairs), size)
    n = len(pair)
    rec = records(pair // nseq, rng.integers(0, 40, n), pair % nseq,
                  rng.integers(0, 40, n), rng.integers(1, 9, n), seqlen)
    rec = rec[rng.permutation(n)]
    layout, kw = layout_of(V, nseq, seqlen)
    opt = dict(kind=kind, value=value, withinborders=True)
    ch = device_of(V, layout, [(rec, False)], **opt)
    same_as_host(V, ch, V.chain_host(layout, rec, **opt), kw)
    st = ch.stats()
    assert (st.problems, st.wave, st.group) == (pairs, 0, 0)
    assert st.single > 5000 and st.tieruns > 0 and st.replayed > 0


# --------------------------------------------------------------------------
# one rule each
# --------------------------------------------------------------------------

def test_equal_priorities_go_to_the_smallest_end1(V):
    # B = record 0 and A = record 1 overlap in dimension 0 and do not chain;
    # both precede C with the score 10.  A has the smaller end0 (4 < 6), B
    # the smaller end1 (7 < 14): B was activated first and stays
    rec = records(0, [2, 0, 20], 0, [3, 10, 20], 5)
    ch, got = run(V, 1, rec, kind=CH.GLOBAL)
    assert chains_of(got) == [(20, [0, 2])]
    # the other way round: the smaller end1 goes with the smaller end0
    rec = records(0, [0, 2, 20], 0, [3, 10, 20], 5)
    ch, got = run(V, 1, rec, kind=CH.GLOBAL)
    assert chains_of(got) == [(20, [0, 2])]
    # equal end1 as well: the smaller number
    rec = np.concatenate([records(0, [2, 0], 0, [3, 3], [5, 5]),
                          records(0, [20], 0, [20], [5])])
    ch, got = run(V, 1, rec, kind=CH.GLOBAL)
    assert chains_of(got) == [(20, [0, 2])]


def test_touching_fragments(V):
    # pair (0, 1): end + 1 = start in both dimensions chains; pair (0, 2):
    # end = start in dimension 1 does not; pair (0, 3): nor in dimension 0
    rec = np.concatenate([records(0, [10, 15], 1, [30, 35], 5),
                          records(0, [10, 15], 2, [30, 34], 5),
                          records(0, [10, 14], 3, [30, 35], 5)])
    # (the local kinds pay the L1 gap (15 - 14) + (35 - 34) for the step)
    for kind, score in ((CH.GLOBAL, 20), (CH.LOCAL_MAX, 18)):
        ch, got = run(V, 4, rec, kind=kind, withinborders=True)
        assert chains_of(got) == [(score, [0, 1]), (10, [2]), (10, [3]),
                                  (10, [4]), (10, [5])]


def test_a_fragment_that_starts_at_zero_has_no_predecessor(V):
    # start0 - 1 must not wrap; in dimension 1 record 0 lies before record
    # 1, which stays alone with the score 6: the threshold 12 leaves it out
    rec = records(0, [0, 0, 4], 0, [0, 10, 20], 3)
    ch, got = run(V, 1, rec, kind=CH.GLOBAL)
    assert chains_of(got) == [(12, [0, 2])]
    ch, got = run(V, 1, rec, kind=CH.GLOBAL_OV)


def test_maxgap_is_asked_of_the_best_candidate_only(V):
    # record 0 (weight 12) and record 1 (weight 10) overlap in dimension 1
    # and do not chain; both precede record 2.  Record 0 is its best
    # predecessor but lies 84 away in dimension 0; record 1 (25 and 47 away)
    # would pass maxgap 50 and is not tried: record 2 stays alone
    rec = records(0, [0, 60, 90], 0, [0, 3, 55], [6, 5, 5])
    ch, got = run(V, 1, rec, kind=CH.GLOBAL, maxgap=50)
    assert chains_of(got) == [(12, [0])]
    ch, got = run(V, 1, rec, kind=CH.GLOBAL, maxgap=90)
    assert chains_of(got) == [(22, [0, 2])]
    ch, got = run(V, 1, rec[1:], kind=CH.GLOBAL, maxgap=50)
    assert chains_of(got) == [(20, [0, 1])]
    # global ov asks every candidate
    ch, got = run(V, 1, rec, kind=CH.GLOBAL_OV, maxgap=50)
    assert chains_of(got) == [(20, [1, 2])]


def test_negative_scores_under_gap_costs(V):
    rec = records(0, [100, 400, 900], 0, [300, 500, 700], 4)
    ch, got = run(V, 1, rec, kind=CH.GLOBAL_GC)
    assert all(s < 0 for s, _ in chains_of(got))
    rec = np.concatenate([rec, records(0, [100], 1, [300], 4)])
    ch, got = run(V, 2, rec, kind=CH.GLOBAL_GC, withinborders=True)
    assert chains_of(got)[-1] == (8 - 100 - (SEQLEN + 1 + 300), [3])


def test_the_weight_is_truncated(V):
    # 0.3 * 14 = 4.2 -> 4, 0.3 * 10 = 3.0 (2.9999... in doubles) -> 2 or 3:
    # whatever the reference's expression gives, on both sides
    rec = records(0, [0, 20, 40], 0, [0, 20, 40], [7, 5, 9])
    ch, got = run(V, 1, rec, kind=CH.GLOBAL, wf=0.3)
    assert chains_of(got) == [(int(0.3 * 14.0) + int(0.3 * 10.0) +
                               int(0.3 * 18.0), [0, 1, 2])]
    assert chains_of(got)[0][0] == 12


def test_the_k_best_distinct_scores(V):
    # five lone fragments with the scores 20, 16, 20, 12, 16: 2b keeps 20
    # and 16, 1b only 20, 9b all
    rec = records(0, [400, 300, 200, 100, 0], 0, [0, 100, 200, 300, 400],
                  [10, 8, 10, 6, 8])
    for k, want in ((1, [20, 20]), (2, [20, 16, 20, 16]),
                    (3, [20, 16, 20, 12, 16]), (9, [20, 16, 20, 12, 16])):
        ch, got = run(V, 1, rec, kind=CH.LOCAL_BEST, value=k)
        assert got["score"].tolist() == want


def test_p_records_from_a_second_add(V):
    rng = np.random.default_rng(41)
    qlen = np.array([40, 93, 64, 17, 128, 55, 80], np.uint64)
    qstart = np.concatenate(([0], np.cumsum(qlen + np.uint64(1))[:-1])) \
        .astype(np.uint64)
    kw = dict(kind=V.SINK_QUERY, totallength=600,
              markpos=np.array([199, 399], np.uint64), querystart=qstart,
              querylength=qlen, querytotallength=int(qstart[-1] + qlen[-1]))
    layout = V.sink_params(**kw)
    n, nd = 2600, 1500
    rec = np.zeros(n, H.MATCH_DTYPE)
    rec["queryseq"] = rng.integers(0, len(qlen), n)
    room = qlen[rec["queryseq"].astype(np.int64)].astype(np.int64)
    rec["length"] = 1 + rng.integers(0, 12, n) % room
    rec["querystart"] = rng.integers(0, 1 << 20, n) % (
        room - rec["length"].astype(np.int64) + 1)
    rec["dbstart"] = rng.integers(0, 3, n) * 200 + rng.integers(0, 180, n)
    flags = (np.arange(n) >= nd).astype(np.uint8)
    for kind, wb in ((CH.LOCAL_MAX, True), (CH.GLOBAL_GC, True),
                     (CH.LOCAL_THRESHOLD, False)):
        opt = dict(kind=kind, value=25, withinborders=wb)
        ch = device_of(V, layout, [(rec[:nd], False), (rec[nd:], True)],
                       **opt)
        host = V.chain_host(layout, rec, palindromic=flags, **opt)
        got = same_as_host(V, ch, host)
        res, pal = ch.records()
        who = got["members"].astype(np.int64)
        assert np.array_equal(res.fetch(), rec[who])
        assert np.array_equal(pal, flags[who]) and pal.any() and not pal.all()
        # the P strand counts from the other end of its query
        plain = V.chain_host(layout, rec, **opt)
        assert not np.array_equal(plain["members"], host["members"])
    # a record that leaves its query is refused, the state stays
    bad = rec[:3].copy()
    bad["querystart"][1] = 1000
    with pytest.raises(V.VsaError) as e:
        ch.add(V.Result.from_host(bad), True)
    assert e.value.code == -2 and "1 records do not fit" in e.value.message
    ch.finish()
    same_as_host(V, ch, host)


def test_the_order_of_the_quicksort_inside_a_tie_run(V):
    # sequence 0 against the sequences 1 .. 4: 6 records each with the same
    # position2, told apart by position1 -- a run of 24 records on seqnum1
    # = 0.  Every problem gives 6 lone chains in the order of its fragments
    rng = np.random.default_rng(8)
    seq2 = np.repeat(np.arange(1, 5), 6)
    rec = records(0, 10 * rng.permutation(24), seq2, np.full(24, 30), 5)
    rec = rec[rng.permutation(24)]
    opt = dict(kind=CH.LOCAL_MAX, withinborders=True)
    ch, got = run(V, 5, rec, **opt)
    st = ch.stats()
    assert (st.tieruns, st.replayed, st.problems, st.chains) == (4, 24, 4, 24)
    layout, kw = layout_of(V, 5)
    stable = CS.as_arrays(model_of(kw, rec, stable=True, **opt))
    assert not np.array_equal(stable["members"], got["members"])
    assert sorted(stable["members"].tolist()) == \
        sorted(got["members"].tolist())
    # ten records on seqnum1 = 0: the insertion sort keeps the order
    few = np.concatenate([rec[seq2[np.argsort(rng.permutation(24))] == 0],
                          rec[:10]])
    ch, got = run(V, 5, few, **opt)
    assert ch.stats().replayed == 0
    stable = CS.as_arrays(model_of(kw, few, stable=True, **opt))
    assert np.array_equal(stable["members"], got["members"])


def test_a_list_without_ties_never_leaves_the_device(V):
    # like the list of -mum: every position2 of a pair is taken once
    rng = np.random.default_rng(9)
    n = 3000
    pair = rng.integers(0, 12, n)
    rec = records(pair // 4, rng.integers(0, 900, n), pair % 4 + 3,
                  rng.permutation(n) % 990, 6)
    _, first = np.unique(np.stack([pair, rec["queryseq"]]), axis=1,
                         return_index=True)
    rec = rec[np.sort(first)]
    ch, got = run(V, 7, rec, kind=CH.LOCAL_THRESHOLD, value=20,
                  withinborders=True)
    st = ch.stats()
    assert (st.tieruns, st.replayed) == (0, 0) and st.group > 0
    assert ch.times()["replay"] == 0.0


def test_positions_above_two_to_the_32(V):
    rng = np.random.default_rng(10)
    seqlen = (1 << 34) + 77
    base = np.uint64((1 << 33) + 5)
    rec = crowded(rng, 0, 0, 500, 3000, seqlen)
    rec["dbstart"] += base
    rec["queryseq"] += base + np.uint64(1 << 32)
    far = crowded(rng, 1, 1, 70, 200, seqlen)
    far["dbstart"] += base
    both = np.concatenate([rec, far])
    for kind in (CH.GLOBAL_GC, CH.LOCAL_MAX, CH.GLOBAL_OV):
        ch, got = run(V, 2, both, seqlen=seqlen, kind=kind,
                      withinborders=True)
        assert ch.stats().problems == 2
        if kind == CH.GLOBAL_GC:
            assert got["score"].min() < -(1 << 33)


def test_nothing_to_chain_and_refusals(V):
    layout, kw = layout_of(V, 2)
    ch = V.Chain(layout, kind=CH.LOCAL_MAX)
    with pytest.raises(V.VsaError) as e:
        ch.chains()                              # not finished yet
    assert e.value.code == -2
    ch.finish()
    assert ch.stats().asdict() == V.chain_host(
        layout, np.zeros(0, H.MATCH_DTYPE))["stats"].asdict()
    assert ch.format(V.Sink(**kw)) == b""
    one = records(0, [5], 1, [7], 9)
    ch.add(V.Result.from_host(one))
    ch.finish()
    assert chains_of(ch.chains()) == [(18, [0])]
    with pytest.raises(V.VsaError) as e:
        ch.add(V.Result.from_host(one), True)    # P under a self layout
    assert e.value.code == V.NOT_COVERED
    assert chains_of(ch.chains()) == [(18, [0])]
    with pytest.raises(V.VsaError) as e:
        V.Chain(layout, thread=True)
    assert e.value.code == V.NOT_COVERED
    sp = V.sink_params(kind=V.SINK_QUERY, totallength=1 << 20,
                       markpos=np.zeros(0, np.uint64), selfpalindromic=True)
    with pytest.raises(V.VsaError) as e:
        V.Chain(sp)
    assert e.value.code == V.NOT_COVERED
