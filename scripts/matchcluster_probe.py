#!/usr/bin/env python3
"""Match clustering at the order of magnitude of the headline's match list:
what vsa_matchcluster_add, _finish and _edges cost on the device, stage by
stage (refs, sort, window, pairs, forest, group), next to what a caller has
to do without them -- vsa_result_fetch of the whole list plus the same rules
on the host (vsa_matchcluster_host).

usage: matchcluster_probe.py [--n N] [--nq NQ] [--m M] [--L L]
                             [--gaps G,G,...] [--pile RECORDS,STARTS ...]
                             [--only mum|pile] [--host-edges LIMIT]
                             [--out FILE]
  mum   the MUM candidates of vmatch -mum cand -l L of NQ reads of M bp on a
        synthetic index of N bp (default 3e9, 1e7, 100, 20: the workload of
        bench.py), clustered with gapsize 0, 100 and 10 000.  position2 of
        such a list is a query coordinate on the axis of position1.
  pile  a synthetic self list of RECORDS matches (default 1e7) whose starts
        are drawn from STARTS places (default 1e5) 1000 symbols apart,
        lengths 30..100, overlap 50: every place is a pile of references
        that all look at each other, the candidate-bound case that takes
        many passes of VSA_MATCHCLUSTER_CHUNK slots.
The host code stores every edge (16 bytes) and sends it through linkcluster:
a case with more than LIMIT edges (default 1e9) is clustered on the device
only, without the group step that brings the edges to the host, and says so.
Prints one JSON line per case (and appends it to FILE): per stage the HIP-event time (vsa_matchcluster_times), per call the wall time
with the host's part and the waits, minimum and median of the runs after one
warm-up run; the fetch and the host clustering; whether the device path
beats fetch plus host, and whether it beats the fetch alone.  Where the host
ran, the device's answer is compared with it.  Needs no reference program.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vstree_amd as V  # noqa: E402

CALLS = ("add", "finish", "edges")


def both(values):
    return dict(min=round(min(values), 3),
                median=round(statistics.median(values), 3))


def host_once(layout, mode, value, rec, flags, nedges):
    """one call of vsa_matchcluster_host with room for the edges the device
    found -> dict like V.matchcluster_host returns, without the text"""
    n = len(rec)
    p = V._matchcluster_params(mode, value)
    st = V.MatchClusterStats()
    cstart = np.zeros(n // 2 + 2, np.uint64)
    estart = np.zeros(n // 2 + 2, np.uint64)
    mem, lab = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    m0, m1 = np.zeros(nedges, np.uint32), np.zeros(nedges, np.uint32)
    val = np.zeros(nedges, np.uint64)
    V._check(V.lib.vsa_matchcluster_host(
        C.byref(layout[0]), C.byref(p), V._ptr(rec), V._ptr(flags), n,
        C.byref(st), V._ptr(cstart), V._ptr(mem), V._ptr(lab),
        V._ptr(estart), V._ptr(m0), V._ptr(m1), V._ptr(val), nedges, None, 0,
        None))
    k = int(st.clusters)
    return dict(stats=st, clusterstart=cstart[:k + 1],
                members=mem[:int(st.inclusters)], labels=lab,
                edgestart=estart[:k + 1], m0=m0, m1=m1, values=val)


def device_run(layout, mode, value, res, grouped=True):
    """grouped: the edges grouped by cluster are brought to the host too (16
    bytes per edge there, twice)"""
    mc = V.MatchCluster(layout, mode, value)
    V.device_synchronize()
    t0 = time.perf_counter()
    mc.add(res)
    t1 = time.perf_counter()
    mc.finish()
    t2 = time.perf_counter()
    edges = mc.edges() if grouped else None
    t3 = time.perf_counter()
    wall = dict(zip(CALLS, ((t1 - t0) * 1e3, (t2 - t1) * 1e3,
                            (t3 - t2) * 1e3)))
    return mc, edges, wall


def probe(name, layout, mode, value, res, host_edges, more):
    """one case -> its JSON record"""
    d = dict(case=name, mode="gapsize" if mode == V.MATCHCLUSTER_GAP
             else "overlap", value=value, matches=res.count, **more)
    try:
        mc, edges, _ = device_run(layout, mode, value, res, False)
        st = mc.stats().asdict()
        grouped = st["edges"] <= host_edges
        if grouped:
            edges = mc.edges()                   # the warm-up run is whole
    except V.VsaError as e:
        d["error"] = "%d: %s" % (e.code, e.message)
        return d
    reps = 3 if st["candidates"] < 5e8 else 1
    ev = {k: [] for k in V.MATCHCLUSTER_STAGES}
    wall = {k: [] for k in CALLS}
    for _ in range(reps):
        mc.close()
        del edges
        mc, edges, w = device_run(layout, mode, value, res, grouped)
        for k, v in mc.times().items():
            ev[k].append(v)
        for k in CALLS:
            wall[k].append(w[k])
    start, members = mc.members()
    labels = mc.labels()
    mc.close()
    fetch = []
    for _ in range(reps):
        t0 = time.perf_counter()
        host = res.fetch()
        fetch.append((time.perf_counter() - t0) * 1e3)
    device = [sum(wall[k][i] for k in CALLS) for i in range(reps)]
    rounds = st.pop("rounds")
    d.update(repeats=reps, stats=st, rounds=rounds,
             chunk=int(os.environ.get("VSA_MATCHCLUSTER_CHUNK", 1 << 26)),
             event_ms={k: both(v) for k, v in ev.items()},
             wall_ms={k: both(v) for k, v in wall.items()},
             device_wall_ms=both(device),
             members_only_wall_ms=both([x + y for x, y in zip(
                 wall["add"], wall["finish"])]),
             fetch_ms=both(fetch), fetch_bytes=32 * res.count,
             device_beats_fetch_alone=bool(
                 statistics.median(device) < statistics.median(fetch)))
    if st["edges"] > host_edges:
        d["host"] = "skipped, and so is the group step (edges): %d edges " \
            "of 16 bytes are more than --host-edges %d" % (st["edges"],
                                                           host_edges)
        return d
    t0 = time.perf_counter()
    want = host_once(layout, mode, value, host,
                     np.zeros(len(host), np.uint8), st["edges"])
    hostms = (time.perf_counter() - t0) * 1e3
    hst = want["stats"].asdict()
    hst.pop("rounds")
    assert st == hst, (st, hst)
    assert np.array_equal(start, want["clusterstart"])
    assert np.array_equal(members, want["members"])
    assert np.array_equal(labels, want["labels"])
    for got, key in zip(edges, ("edgestart", "m0", "m1", "values")):
        assert np.array_equal(got, want[key]), key
    parent = statistics.median(fetch) + hostms
    d.update(host_cluster_ms=round(hostms, 3), parent_ms=round(parent, 3),
             ratio_parent_over_device=round(
                 parent / statistics.median(device), 2),
             equal_to_host=True)
    return d


def mum_list(n, nq, m, L):
    """the headline's list and its layout; the index is freed again"""
    dg = V.device_malloc(n + 64)
    V._check(V.lib.vsa_synth_genome_device(V.GENOME_SEED, n, dg, 0))
    index = V.Index.build_device(dg, n, 4, 0)
    pos, sub, step = V.synth_query_plan(n, nq, m)
    dq = V.device_malloc(nq * m + 64)
    V._check(V.lib.vsa_synth_queries_device(
        dg, n, pos.ctypes.data, sub.ctypes.data, step.ctypes.data, nq, m,
        dq, 0))
    queries = V.Queries.from_device(dq, nq, m)
    res = V.findquerymatches(index, queries, L, mum=True, cand=True)
    index.close()
    layout = V.sink_params(
        kind=V.SINK_QUERY, totallength=n, markpos=[],
        querystart=np.arange(nq, dtype=np.uint64) * np.uint64(m + 1),
        querylength=np.full(nq, m, np.uint64),
        querytotallength=nq * (m + 1) - 1, leastlength=L)
    return res, layout


def pile_list(nrec, nstarts, seed=11):
    rng = np.random.default_rng(seed)
    rec = np.zeros(nrec, V.MATCH_DTYPE)
    rec["length"] = rng.integers(30, 101, nrec)
    rec["dbstart"] = rng.integers(0, nstarts, nrec) * 1000
    rec["queryseq"] = rng.integers(0, nstarts, nrec) * 1000
    layout = V.sink_params(kind=V.SINK_SELF, totallength=nstarts * 1000,
                           markpos=[])
    return V.Result.from_host(rec), layout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=3e9)
    ap.add_argument("--nq", type=float, default=1e7)
    ap.add_argument("--m", type=int, default=100)
    ap.add_argument("--L", type=int, default=20)
    ap.add_argument("--gaps", default="0,100,10000")
    ap.add_argument("--pile", action="append", default=None)
    ap.add_argument("--only", choices=("mum", "pile"), default=None)
    ap.add_argument("--host-edges", type=float, default=1e9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if V.device_count() < 1:
        sys.exit("matchcluster_probe.py needs a GPU")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def report(d):
        print(json.dumps(d), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(d) + "\n")

    limit = int(a.host_edges)
    if a.only != "mum":
        for spec in a.pile or ["1e7,1e5"]:
            nrec, nstarts = (int(float(x)) for x in spec.split(","))
            res, layout = pile_list(nrec, nstarts)
            report(probe("pile", layout, V.MATCHCLUSTER_OVERLAP, 50, res,
                         limit, dict(starts=nstarts)))
            res.close()
    if a.only != "pile":
        n, nq, m, L = int(a.n), int(a.nq), a.m, a.L
        res, layout = mum_list(n, nq, m, L)
        for G in (int(x) for x in a.gaps.split(",")):
            report(probe("mum", layout, V.MATCHCLUSTER_GAP, G, res, limit,
                         dict(n=n, nq=nq, m=m, L=L)))


if __name__ == "__main__":
    main()
