#!/usr/bin/env python3
"""The X-drop extension of exact seeds (vmatch -l L -hxdrop X | -exdrop X) on
two workloads, next to what a caller has to do without it -- the fetch of the
seed list plus vsa_extend_xdrop_host on 16 threads, timed in the same run:

  reads  NQ reads of M symbols, SUBST substitutions each and one insertion or
         deletion in every second read, against a random index of N symbols,
         -l 60 -seedlength 20 -q
  self   a random text of N symbols with planted repeat families of 2-10 %
         divergence against itself, -l 100 (seeds of 30 symbols)

each with -hxdrop and -exdrop at X = 5 and X = 20.

usage: extend_xdrop_probe.py [N [NQ [M]]] [--only reads|self] [--out FILE]
       (default 1e8, 1e7, 150; FILE default
       profiles/r22/extend_xdrop_probe.json)

Per workload and parameter set one JSON object: seeds, matches, seeds per
second, the sides the long stage scanned / with a slide the group finished,
the seeds handed over to the host rules, the HIP-event times (best of three
calls, after one call that is not timed), the time of the seed search and the
host figures.  The device list is compared with the host's.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import vstree_amd as V  # noqa: E402
from extend_probe import substituted_reads, planted_text  # noqa: E402
from extend_edist_probe import with_indels  # noqa: E402

HOST_THREADS = 16
REPEAT = 3
PARAMS = ((True, 5), (True, 20), (False, 5), (False, 20))


def measure(name, index, text, seeds, L, X, hamming, S, queries, hostqueries,
            search_ms):
    V.extend_xdrop(index, queries, seeds, L, X, S, hamming=hamming).close()
    best = None
    for _ in range(REPEAT):
        res = V.extend_xdrop(index, queries, seeds, L, X, S, hamming=hamming)
        st = res.stats()
        if best is None or st.search_kernel_ms < best[1].search_kernel_ms:
            best = (res, st)
    res, st = best
    got = res.fetch()
    nseeds = seeds.count
    t0 = time.time()
    hostseeds = seeds.fetch()
    t1 = time.time()
    host = V.extend_xdrop_host(text, hostseeds, L, X, S, queries=hostqueries,
                               threads=HOST_THREADS, hamming=hamming)
    t2 = time.time()
    same = bool(np.array_equal(got, host))
    out = dict(
        workload=name, option="-hxdrop" if hamming else "-exdrop", xdrop=X,
        leastlength=L, seedlength=V.extend_xdrop_seedlength(S), seeds=nseeds,
        matches=int(st.count),
        matches_of_unequal_lengths=int((V.xdrop_lengths1(got) !=
                                        V.xdrop_lengths2(got)).sum()),
        cooperative_sides=int(st.searches),
        handed_over_seeds=int(st.kernel_searches),
        seed_search_ms=search_ms, extension_ms=st.search_kernel_ms,
        first_stage_ms=st.first_kernel_ms, later_stages_ms=st.anchor_ms,
        call_device_ms=st.total_device_ms,
        seeds_per_second=nseeds / max(st.total_device_ms, 1e-9) * 1e3,
        repetitions=REPEAT, warm_calls=1,
        host_threads=HOST_THREADS, seed_fetch_ms=(t1 - t0) * 1e3,
        host_extension_ms=(t2 - t1) * 1e3,
        fetch_plus_host_ms=(t2 - t0) * 1e3,
        fetch_plus_host_over_device=(t2 - t0) * 1e3 /
        max(st.total_device_ms, 1e-9),
        device_equals_host=same)
    print(json.dumps(out), flush=True)
    assert same, name
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="?", type=float, default=1e8)
    ap.add_argument("nq", nargs="?", type=float, default=1e7)
    ap.add_argument("m", nargs="?", type=int, default=150)
    ap.add_argument("--subst", type=int, default=2)
    ap.add_argument("--only", choices=("reads", "self"), default=None)
    ap.add_argument("--out", default=os.path.join(
        ROOT, "profiles", "r22", "extend_xdrop_probe.json"))
    a = ap.parse_args()
    n, nq, m = int(a.n), int(a.nq), a.m
    rng = np.random.default_rng(22)
    results = []
    if a.only != "self":
        genome = V.synth_genome(n)
        index = V.Index.build(genome, 4, 0, 0)
        reads = with_indels(rng, substituted_reads(rng, genome, nq, m,
                                                   a.subst), nq, m)
        dq = V.device_malloc(nq * m + 64)
        V.device_upload(dq, reads)
        queries = V.Queries.from_device(dq, nq, m)
        L, S = 60, 20
        V.findquerymatches(index, queries, S).close()
        V.device_synchronize()
        t0 = time.time()
        seeds = V.findquerymatches(index, queries, S)
        search_ms = (time.time() - t0) * 1e3
        hostq = (reads, np.arange(nq, dtype=np.uint64) * np.uint64(m),
                 np.full(nq, m, np.uint64))
        for hamming, X in PARAMS:
            results.append(measure("reads", index, genome, seeds, L, X,
                                   hamming, S, queries, hostq, search_ms))
        seeds.close()
        queries.close()
        V.device_free(dq)
        index.close()
    if a.only != "reads":
        text = planted_text(rng, n, max(1, n // 50000), 6, 2000)
        index = V.Index.build(text, 4, 0, 0)
        L, S = 100, 0
        V.device_synchronize()
        t0 = time.time()
        seeds = V.findmaximalrepeats(index, V.extend_xdrop_seedlength(S))
        search_ms = (time.time() - t0) * 1e3
        for hamming, X in PARAMS:
            results.append(measure("self", index, text, seeds, L, X, hamming,
                                   S, None, None, search_ms))
        seeds.close()
        index.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(n=n, nq=nq, m=m, subst=a.subst, results=results), f,
                  indent=1)


if __name__ == "__main__":
    main()
