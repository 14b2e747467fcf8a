"""The list that select, cluster, matchcluster (gapsize and erate) and chain
accumulate in device memory over their add calls (resident_list.hpp): 773
records, three tiles of 256 and five, fed to a fresh handle in adds of 1, 1,
2, 4, ... 256 records and the remaining 261, so that every doubling of the
capacity from 1 upward moves live records.  Between two of the adds a list
is refused that would have made the handle grow.  Every output must equal,
element for element and byte for byte, that of a handle fed the 773 records
in one add and that of the host twin; then 300 more records and a second
finish, against both again."""
import numpy as np
import pytest

import helpers as H
import chain_model as CH
import cluster_cases as CC
import erate_cases as EC
import matchcluster_cases as MC
import matchcluster_model as MM
import select_model as SM
import test_gpu_chain as TCH
import test_gpu_cluster as TCL
import test_gpu_matchcluster as TMC
import test_gpu_matchcluster_erate as TER
from test_gpu_select import ragged_batch

pytestmark = pytest.mark.gpu

N, MORE = 773, 300
ADDS = [1, 1, 2, 4, 8, 16, 32, 64, 128, 256, N - 512]
REFUSE_AFTER = 7          # 64 records are in: one more needs a larger list
assert sum(ADDS) == N and sum(ADDS[:REFUSE_AFTER]) == 64


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


class Select:
    """filters only, against queries, the P strand"""

    def __init__(self, V):
        rng = np.random.default_rng(21)
        self.V = V
        lengths = 40 + np.arange(9, dtype=np.uint64)
        start = np.concatenate(([0], np.cumsum(lengths + np.uint64(1))[:-1]))
        total = int(lengths.sum()) + len(lengths) - 1
        self.lengths = lengths
        self.layout = V.sink_params(kind=SM.QUERY, totallength=10 ** 6,
                                    markpos=[], leastlength=12,
                                    querystart=start, querylength=lengths,
                                    querytotallength=total)
        n = N + MORE
        rec = np.zeros(n, H.MATCH_DTYPE)
        rec["queryseq"] = rng.integers(0, len(lengths), n)
        rec["length"] = rng.integers(8, 21, n)       # below 12: filtered
        rec["querystart"] = rng.integers(0, 20, n)
        rec["dbstart"] = rng.integers(0, 10 ** 6 - 20, n)
        self.rec = rec
        self.flags = np.ones(n, np.uint8)
        # a query number outside the batch, in a list that would not fit
        self.bad = rec[:N].copy()
        self.bad["queryseq"][500] = len(lengths)

    def open(self):
        return self.V.Select(self.layout, ragged_batch(self.V,
                                                       self.lengths)[0])

    def add(self, h, a, b):
        h.add(self.V.Result.from_host(self.rec[a:b]), True)

    def refuse(self, h):
        h.add(self.V.Result.from_host(self.bad))

    def outputs(self, h):
        got = h.finish().fetch()
        return dict(records=got, flags=h.flags(len(got)),
                    stats=h.stats().asdict())

    def host(self, n):
        rec, flags, _, st = self.V.select_host(self.layout, self.rec[:n],
                                               self.flags[:n])
        assert 0 < len(rec) < n and flags.all()
        return dict(records=rec, flags=flags, stats=st.asdict())

    def against_host(self, h, n):
        same(self.outputs(h), self.host(n))


class Cluster:
    def __init__(self, V):
        rng = np.random.default_rng(22)
        self.V = V
        self.layout, _ = CC.synthetic_layout(V, TCL.NSEQ, TCL.SEQLEN)
        pairs = rng.integers(0, TCL.NSEQ // 2, (N + MORE, 2)) * 2
        pairs[:, 1] += 1                         # never the same sequence
        self.rec = CC.self_records(TCL.SEQLEN, pairs)
        self.flags = np.zeros(N + MORE, np.uint8)
        self.bad = self.rec[:1].copy()
        self.bad["length"] = TCL.SEQLEN + 1      # it leaves its sequence

    def open(self):
        return self.V.Cluster(self.layout, 50, 50)

    def add(self, h, a, b):
        h.add(self.V.Result.from_host(self.rec[a:b]))

    def refuse(self, h):
        # every record so far is an edge: the list is full
        assert h.stats().edges == h.stats().seen == 64
        h.add(self.V.Result.from_host(self.bad))

    def outputs(self, h):
        start, mem = h.members()
        res, eflags, estart = h.edges()
        return dict(stats=h.stats().asdict(), clusterstart=start, members=mem,
                    labels=h.labels(), text=h.format(), edges=res.fetch(),
                    edgeflags=eflags, edgestart=estart)

    def host(self, n):
        host = self.V.cluster_host(self.layout, 50, 50, self.rec[:n],
                                   self.flags[:n])
        host["stats"] = host["stats"].asdict()
        assert host["stats"]["edges"] == n
        return host

    def against_host(self, h, n):
        TCL.compare(h, self.host(n), self.rec[:n], self.flags[:n])


class MatchCluster:
    """gapsize"""

    def __init__(self, V):
        rng = np.random.default_rng(23)
        self.V = V
        self.layout = MC.synthetic_layout(V)
        self.sink = V.Sink(kind=2, totallength=1 << 20,
                           markpos=np.zeros(0, np.uint64))
        n = N + MORE
        places = rng.integers(0, 20000, 400)
        self.rec = MC.records(rng.integers(1, 60, n), rng.choice(places, n),
                              rng.choice(places, n))
        # it lies outside its sequence, the only one of the text
        self.bad = MC.records(10, [100], [1 << 21])

    def open(self):
        return self.V.MatchCluster(self.layout, MM.GAP, 30)

    def add(self, h, a, b):
        h.add(self.V.Result.from_host(self.rec[a:b]))

    def refuse(self, h):
        h.add(self.V.Result.from_host(self.bad))

    def outputs(self, h):
        start, mem = h.members()
        estart, m0, m1, values = h.edges()
        res, flags = h.records()
        texts = [h.format_cluster(self.sink, c, start[c + 1] - start[c],
                                  estart[c + 1] - estart[c])
                 for c in range(len(start) - 1)]
        return dict(stats=h.stats().asdict(), clusterstart=start, members=mem,
                    labels=h.labels(), text=h.format(), edgestart=estart,
                    m0=m0, m1=m1, values=values, records=res.fetch(),
                    flags=flags, clustertexts=texts)

    def host(self, n):
        return self.V.matchcluster_host(self.layout, MM.GAP, 30, self.rec[:n])

    def against_host(self, h, n):
        host = self.host(n)
        assert host["stats"].edges > 256         # more than a tile of them
        self.compare(h, host, self.rec[:n])
        got = self.outputs(h)
        start, estart = got["clusterstart"], got["edgestart"]
        for c, text in enumerate(got["clustertexts"]):
            mem = got["members"][int(start[c]):int(start[c + 1])]
            e = slice(int(estart[c]), int(estart[c + 1]))
            assert text == self.V.matchcluster_format_host(
                self.sink, h.mode, mem, self.rec[mem.astype(np.int64)],
                got["m0"][e], got["m1"][e], got["values"][e])

    def compare(self, h, host, rec):
        host = dict(host, stats=host["stats"].asdict())
        TMC.compare(h, host, rec)


class ErateCluster(MatchCluster):
    def __init__(self, V):
        self.V = V
        self.text, self.rec = EC.planted_list(33, n=N + MORE)
        self.layout = EC.layout_of(V, self.text)
        self.sink = V.Sink(kind=2, totallength=len(self.text),
                           markpos=np.flatnonzero(self.text == H.SEPARATOR)
                           .astype(np.uint64))
        self.bad = EC.records(30, [int(self.rec["dbstart"][0])],
                              [len(self.text) - 10])     # it leaves the text

    def open(self):
        return self.V.MatchCluster.erate(
            self.layout, TER.index_of(self.V, "planted33", self.text), 10)

    def host(self, n):
        return self.V.matchcluster_erate_host(self.layout, 10, self.text,
                                              self.rec[:n])

    def compare(self, h, host, rec):
        TER.compare(self.V, h, host, rec, self.sink)


class Chain:
    OPT = dict(kind=CH.LOCAL_MAX, withinborders=True)

    def __init__(self, V):
        rng = np.random.default_rng(24)
        self.V = V
        sizes = [1, 9, 65, 300, 398, MORE]       # one problem per pair
        assert sum(sizes) == N + MORE
        self.layout, self.kw = TCH.layout_of(V, len(sizes) + 1)
        rec = np.concatenate([TCH.crowded(rng, p, p + 1, n,
                                          min(8 + 2 * n, 900))
                              for p, n in enumerate(sizes)])
        self.rec = np.concatenate([rec[:N][rng.permutation(N)], rec[N:]])
        self.bad = TCH.records(0, [TCH.SEQLEN - 5], 1, [5], 10)

    def open(self):
        return self.V.Chain(self.layout, **self.OPT)

    def add(self, h, a, b):
        h.add(self.V.Result.from_host(self.rec[a:b]))

    def refuse(self, h):
        h.add(self.V.Result.from_host(self.bad))

    def outputs(self, h):
        res, flags = h.records()
        return dict(h.chains(), stats=h.stats().asdict(), records=res.fetch(),
                    flags=flags, text=h.format(self.V.Sink(**self.kw)))

    def host(self, n):
        host = self.V.chain_host(self.layout, self.rec[:n], **self.OPT)
        assert host["stats"].problems == (5 if n == N else 6)
        return host

    def against_host(self, h, n):
        host = self.host(n)
        got = TCH.same_as_host(self.V, h, host, self.kw)
        assert np.array_equal(h.records()[0].fetch(),
                              self.rec[:n][got["members"].astype(np.int64)])


@pytest.mark.parametrize("user", [Select, Cluster, MatchCluster, ErateCluster,
                                  Chain])
def test_a_list_that_grows_under_live_records(V, user):
    u = user(V)
    h, a = u.open(), 0
    for k, m in enumerate(ADDS):
        if k == REFUSE_AFTER:
            before = h.stats().asdict()
            with pytest.raises(V.VsaError) as e:
                u.refuse(h)
            assert e.value.code == -2
            assert h.stats().asdict() == before
        u.add(h, a, a + m)
        a += m
    if user is not Select:
        h.finish()
        one = u.open()
        u.add(one, 0, N)
        one.finish()
    else:
        one = u.open()
        u.add(one, 0, N)
    same(u.outputs(h), u.outputs(one))
    u.against_host(h, N)
    # finish, add more, finish: the list grew in between
    u.add(h, N, N + MORE)
    two = u.open()
    u.add(two, 0, N + MORE)
    if user is not Select:
        h.finish()
        two.finish()
    same(u.outputs(h), u.outputs(two))
    u.against_host(h, N + MORE)
