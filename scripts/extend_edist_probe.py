#!/usr/bin/env python3
"""The edit-distance extension of exact seeds (vmatch -l L -e K outside
-complete) on two workloads, next to what a caller has to do without it --
the fetch of the seed list plus vsa_extend_edist_host on 16 threads, timed in
the same run -- and, for context, the Hamming extension of the same seeds:

  reads  NQ reads of M symbols, SUBST substitutions each and one insertion or
         deletion in every second read, against a random index of N symbols,
         -l 60 -e 3 -q  (seed length 15)
  self   a random text of N symbols with planted repeat families of 2-10 %
         divergence against itself, -l 100 -e 5 -seedlength 20

usage: extend_edist_probe.py [N [NQ [M]]] [--only reads|self] [--out FILE]
       (default 1e8, 1e7, 150; FILE default
       profiles/r20/extend_edist_probe.json)

Per workload one JSON object: seeds, matches, the matches whose instances
differ in length, the share of sides with a slide the group finished
together, the scratch bytes per seed, the HIP-event times (best of three
calls, after one call that is not timed; every call makes its scratch anew
from the library's cache), the time of the seed search, the Hamming figures
and the host figures.  The device list is compared with the host's.
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

HOST_THREADS = 16
REPEAT = 3


def with_indels(rng, reads, nq, m):
    """every second read: one symbol inserted or deleted at a random place,
    the length kept (the tail moves)"""
    block = reads.reshape(nq, m)
    for a in range(0, nq, 2 << 20):
        rows = np.arange(a, min(nq, a + (2 << 20)), 2)
        at = rng.integers(10, m - 10, len(rows))
        ins = rng.random(len(rows)) < 0.5
        col = np.arange(m)[None, :]
        src = np.where(ins[:, None], np.where(col > at[:, None], col - 1, col),
                       np.where(col >= at[:, None],
                                np.minimum(col + 1, m - 1), col))
        block[rows] = block[rows[:, None], src]
    return block.reshape(-1)


def measure(name, index, text, seeds, L, K, S, queries, hostqueries,
            search_ms):
    V.extend_edist(index, queries, seeds, L, K, S).close()
    best = None
    for _ in range(REPEAT):
        res = V.extend_edist(index, queries, seeds, L, K, S)
        st = res.stats()
        if best is None or st.search_kernel_ms < best[1].search_kernel_ms:
            best = (res, st)
    res, st = best
    got = res.fetch()
    hbest = None
    V.extend_hamming(index, queries, seeds, L, K, S).close()
    for _ in range(REPEAT):
        hst = V.extend_hamming(index, queries, seeds, L, K, S).stats()
        if hbest is None or hst.search_kernel_ms < hbest.search_kernel_ms:
            hbest = hst
    nseeds = seeds.count
    t0 = time.time()
    hostseeds = seeds.fetch()
    t1 = time.time()
    host = V.extend_edist_host(text, hostseeds, L, K, S, queries=hostqueries,
                               threads=HOST_THREADS)
    t2 = time.time()
    same = bool(np.array_equal(got, host))
    out = dict(
        workload=name, leastlength=L, maxdist=K,
        seedlength=V.extend_seedlength(L, K, S), seeds=nseeds,
        matches=int(st.count),
        matches_of_unequal_lengths=int((V.edist_lengths1(got) !=
                                        V.edist_lengths2(got)).sum()),
        cooperative_sides=int(st.searches),
        cooperative_share_of_sides=st.searches / (2.0 * max(1, nseeds)),
        scratch_bytes_per_seed=8 * (K + 1) ** 2,
        seed_search_ms=search_ms, extension_ms=st.search_kernel_ms,
        fronts_ms=st.first_kernel_ms,
        choice_ms=st.search_kernel_ms - st.first_kernel_ms,
        call_device_ms=st.total_device_ms, repetitions=REPEAT, warm_calls=1,
        hamming_extension_ms=hbest.search_kernel_ms,
        hamming_matches=int(hbest.count),
        host_threads=HOST_THREADS, seed_fetch_ms=(t1 - t0) * 1e3,
        host_extension_ms=(t2 - t1) * 1e3,
        fetch_plus_host_ms=(t2 - t0) * 1e3,
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
        ROOT, "profiles", "r20", "extend_edist_probe.json"))
    a = ap.parse_args()
    n, nq, m = int(a.n), int(a.nq), a.m
    rng = np.random.default_rng(20)
    results = []
    if a.only != "self":
        genome = V.synth_genome(n)
        index = V.Index.build(genome, 4, 0, 0)
        reads = with_indels(rng, substituted_reads(rng, genome, nq, m,
                                                   a.subst), nq, m)
        dq = V.device_malloc(nq * m + 64)
        V.device_upload(dq, reads)
        queries = V.Queries.from_device(dq, nq, m)
        L, K, S = 60, 3, 0
        V.findquerymatches(index, queries, V.extend_seedlength(L, K, S)).close()
        V.device_synchronize()
        t0 = time.time()
        seeds = V.findquerymatches(index, queries,
                                   V.extend_seedlength(L, K, S))
        search_ms = (time.time() - t0) * 1e3
        hostq = (reads, np.arange(nq, dtype=np.uint64) * np.uint64(m),
                 np.full(nq, m, np.uint64))
        results.append(measure("reads", index, genome, seeds, L, K, S,
                               queries, hostq, search_ms))
        seeds.close()
        queries.close()
        V.device_free(dq)
        index.close()
    if a.only != "reads":
        text = planted_text(rng, n, max(1, n // 50000), 6, 2000)
        index = V.Index.build(text, 4, 0, 0)
        L, K, S = 100, 5, 20
        V.device_synchronize()
        t0 = time.time()
        seeds = V.findmaximalrepeats(index, V.extend_seedlength(L, K, S))
        search_ms = (time.time() - t0) * 1e3
        results.append(measure("self", index, text, seeds, L, K, S, None,
                               None, search_ms))
        seeds.close()
        index.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(n=n, nq=nq, m=m, subst=a.subst, results=results), f,
                  indent=1)


if __name__ == "__main__":
    main()
