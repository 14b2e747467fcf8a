"""Chaining without a GPU: the pure-Python model (chain_model.py) in both of
its forms -- the literal sweep and the rule without an order of events --,
vsa_chain_host and vsa_chain_format_host against the recorded runs of the
real reference (chain table, members, the md5 of the printed text), the rule
against the sweep and against the host code on random problems with crowded
coordinates, the restated quicksort of the grouping, and the refusals."""
import numpy as np
import pytest

import helpers as H
import chain_cases as CS
import chain_model as CH
import matchcluster_cases as MC
import vstree_amd as V


def host_of(layout, rec, flags=None, **options):
    got = V.chain_host(layout, rec, palindromic=flags, **options)
    got["stats"] = got["stats"].asdict()
    return got


def same(got, want):
    """got: arrays of the library; want: what chain_model.chain returns"""
    assert got["stats"] == want["stats"]
    arr = CS.as_arrays(want)
    for k in arr:
        assert np.array_equal(got[k], arr[k]), k


@pytest.mark.parametrize("key", CS.keys())
def test_recorded_runs(key):
    r = CS.run_of(key)
    rec, flags = CS.input_of(key)
    layout = V.sink_params(**CS.layout_kwargs(r))
    lines = CS.lines_of(V, r, rec, flags)
    host = host_of(layout, rec, flags if flags.any() else None,
                   **CS.options(r))
    CS.check_against_manifest(key, host["stats"], host,
                              CS.text_of(host, lines, r["silent"]))
    for form in ("sweep", "rule"):
        want = CS.model_of(r, rec, flags, form=form)
        same(host, want)
        arr = CS.as_arrays(want)
        CS.check_against_manifest(key, want["stats"], arr,
                                  CS.text_of(arr, lines, r["silent"]))
    if not flags.any():
        # one pass: the library's own formatter prints the same text
        sink = V.Sink(**CS.layout_kwargs(r))
        who = host["members"].astype(np.int64)
        text = V.chain_format_host(sink, host["number"], host["score"],
                                   host["start"], rec[who],
                                   silent=r["silent"])
        assert CS.md5(text) == CS.manifest()["runs"][key]["md5_text"]


def test_the_quicksort_order_shows_in_a_recorded_run():
    shown = CS.manifest()["order_matters"]
    assert shown and set(shown) <= set(CS.keys())
    for key in shown:
        r = CS.run_of(key)
        rec, flags = CS.input_of(key)
        want = CS.as_arrays(CS.model_of(r, rec, flags))
        stable = CS.as_arrays(CS.model_of(r, rec, flags, stable=True))
        assert not np.array_equal(want["members"], stable["members"])


def random_problem(rng, span):
    n = int(rng.integers(2, 41))
    len1 = rng.integers(1, max(2, span // 3) + 1, n)
    len2 = rng.integers(1, max(2, span // 3) + 1, n)
    pos1 = rng.integers(0, span + 1, n)
    pos2 = rng.integers(0, span + 1, n)
    return len1.tolist(), pos1.tolist(), len2.tolist(), pos2.tolist()


KINDS = [(CH.GLOBAL, 0), (CH.GLOBAL_GC, 0), (CH.GLOBAL_OV, 0),
         (CH.LOCAL_MAX, 0), (CH.LOCAL_THRESHOLD, 9), (CH.LOCAL_BEST, 2),
         (CH.LOCAL_PERCENT, 30)]


def test_rule_against_literal_sweep_on_random_problems():
    rng = np.random.default_rng(20261019)
    ties = 0
    for k in range(2100):
        span = (12, 40, 200)[k % 3]
        kind, value = KINDS[k % len(KINDS)]
        maxgap = 0 if (k // 21) % 2 == 0 else int(rng.integers(1, span))
        wf = (1.0, 0.3)[(k // 7) % 2]
        l1, p1, l2, p2 = random_problem(rng, span)
        zeros = [0] * len(l1)
        got = {form: CH.chain(l1, p1, l2, p2, zeros, zeros, kind, value,
                              maxgap, wf, form=form)
               for form in ("sweep", "rule")}
        assert got["sweep"]["chains"] == got["rule"]["chains"], k
        assert got["sweep"]["members"] == got["rule"]["members"], k
        ties += got["sweep"]["stats"]["tieruns"]
    assert ties > 1000


def test_host_against_the_model_on_random_lists():
    rng = np.random.default_rng(77)
    nseq, seqlen = 6, 260
    total = nseq * (seqlen + 1) - 1
    markpos = np.arange(1, nseq, dtype=np.uint64) * np.uint64(seqlen + 1) - \
        np.uint64(1)
    layout = V.sink_params(kind=2, totallength=total, markpos=markpos)
    chains = 0
    for k in range(280):
        kind, value = KINDS[k % len(KINDS)]
        n = int(rng.integers(0, 120))
        span = (12, 40, 200)[k % 3]
        s1 = rng.integers(0, nseq if k % 5 else 2, n)
        s2 = rng.integers(0, nseq if k % 5 else 2, n)
        length = rng.integers(1, 20, n)
        rel1 = rng.integers(0, span + 1, n)
        rel2 = rng.integers(0, span + 1, n)
        rec = np.zeros(n, H.MATCH_DTYPE)
        rec["length"] = length
        rec["dbstart"] = s1 * (seqlen + 1) + rel1
        rec["queryseq"] = s2 * (seqlen + 1) + rel2
        opt = dict(kind=kind, value=value,
                   maxgap=0 if k % 2 else int(rng.integers(1, span)),
                   wf=(1.0, 0.3)[(k // 7) % 2], withinborders=k % 3 != 0)
        got = host_of(layout, rec, **opt)
        l1 = length.tolist()
        for form in ("sweep", "rule"):
            want = CH.chain(l1, rec["dbstart"].tolist(), l1,
                            rec["queryseq"].tolist(), s1.tolist(),
                            s2.tolist(), form=form, **opt)
            same(got, want)
        chains += got["stats"]["chains"]
    assert chains > 3000


def test_the_restated_quicksort():
    rng = np.random.default_rng(5)
    shuffled = 0
    for n in (1, 2, 3, 10, 11, 12, 40, 300):
        for distinct in (1, 2, 5, 1000):
            key = rng.integers(0, distinct, n).tolist()
            perm = list(range(n))
            CH.quicksort(perm, 0, n - 1, key)
            assert sorted(perm) == list(range(n))
            assert [key[m] for m in perm] == sorted(key)
            stable = sorted(range(n), key=lambda m: key[m])
            if n <= 10:
                assert perm == stable
            shuffled += perm != stable
    assert shuffled > 0


def test_small_lists_and_refusals():
    layout = MC.synthetic_layout(V)
    rec = MC.records([10, 10], [0, 100], [50, 150])
    for kind, value in KINDS:
        got = host_of(layout, rec[:0], kind=kind, value=value)
        assert got["stats"]["chains"] == 0 and got["stats"]["problems"] == 0
        # one fragment is a chain whatever the threshold
        got = host_of(layout, rec[:1], kind=kind, value=max(value, 1) * 1000)
        assert got["members"].tolist() == [0]
        assert got["score"].tolist() == [20 - (50 if kind == CH.GLOBAL_GC
                                                else 0)]
    with pytest.raises(V.VsaError) as e:
        V.chain_host(layout, rec, thread=True)
    assert e.value.code == V.NOT_COVERED and "thread" in e.value.message
    pal = V.sink_params(kind=1, totallength=1 << 20,
                        markpos=np.zeros(0, np.uint64), selfpalindromic=True,
                        palindromic=True)
    with pytest.raises(V.VsaError) as e:
        V.chain_host(pal, rec)
    assert e.value.code == V.NOT_COVERED
    with pytest.raises(V.VsaError) as e:
        V.chain_host(layout, rec, palindromic=[0, 1])
    assert e.value.code == V.NOT_COVERED
    for bad in (dict(kind=7), dict(wf=0.0), dict(kind=CH.LOCAL_BEST, value=0)):
        with pytest.raises(V.VsaError) as e:
            V.chain_host(layout, rec, **bad)
        assert e.value.code == -2
    outside = rec.copy()
    outside["queryseq"][1] = 1 << 21
    with pytest.raises(V.VsaError) as e:
        V.chain_host(layout, outside)
    assert e.value.code == -2 and "record 1" in e.value.message


def test_abi_names():
    syms = {s for s in V.ABI_SYMBOLS if s.startswith("vsa_chain_")}
    assert len(syms) == 12
    assert V.CHAIN_MAXGROUP == 1 << 15
