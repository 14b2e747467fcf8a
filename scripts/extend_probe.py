#!/usr/bin/env python3
"""The Hamming extension of exact seeds (vmatch -l L -h K outside -complete)
on two workloads, next to what a caller has to do without it -- the fetch of
the seed list plus vsa_extend_hamming_host on 16 threads, timed in the same
run:

  reads  NQ reads of M symbols, SUBST substitutions each, against a random
         index of N symbols, -l 100 -h 3 -q  (seed length 25)
  self   a random text of N symbols with planted repeat families of 2-10 %
         divergence against itself, -l 100 -h 5 -seedlength 20

usage: extend_probe.py [N [NQ [M]]] [--only reads|self] [--out FILE]
       (default 1e8, 1e7, 150; FILE default profiles/r18/extend_probe.json)

Per workload one JSON object: seeds, matches, the share of sides the long
stage scanned, the HIP-event times of the stages (best of three calls), the
bytes per seed the stages move AT LEAST -- counted from the lists, not
measured: the records, the tables, the flags and the symbols between the
seeds and the ends of their matches, in both texts -- that over the time of
the extension as a fraction of the streaming read rate measured in the same
run (vsa_measure_stream_read), the time of the seed search, and the host
figures.  The device list is compared with the host's.

Seed lengths below 20 are the caller's budget: at 32 bytes a seed and
hundreds of seeds a read the seed list itself is what fills HBM.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vstree_amd as V  # noqa: E402

HOST_THREADS = 16


def substituted_reads(rng, genome, nq, m, nsubst, chunk=1 << 20):
    """nq windows of m symbols with nsubst substitutions at distinct places"""
    n = len(genome)
    out = np.empty(nq * m, np.uint8)
    for a in range(0, nq, chunk):
        b = min(nq, a + chunk)
        pos = rng.integers(0, n - m, b - a)
        block = genome[pos[:, None] + np.arange(m, dtype=np.int64)[None, :]]
        # distinct places: a sorted draw from m - nsubst + 1, spread by rank
        places = np.sort(rng.integers(0, m - nsubst + 1, (b - a, nsubst)),
                         axis=1) + np.arange(nsubst)[None, :]
        rows = np.arange(b - a)[:, None]
        block[rows, places] = (block[rows, places] + 1 +
                               rng.integers(0, 3, (b - a, nsubst))) % 4
        out[a * m:b * m] = block.reshape(-1)
    return out


def planted_text(rng, n, families, members, length):
    """a random text with `families` groups of `members` diverged copies of a
    segment of `length` symbols, 2-10 % substitutions per copy"""
    text = rng.integers(0, 4, n).astype(np.uint8)
    slots = rng.permutation(n // (length + 64) - 1)[:families * members]
    for f in range(families):
        src = text[int(slots[f * members]) * (length + 64):][:length].copy()
        for k in range(1, members):
            copy = src.copy()
            d = rng.uniform(0.02, 0.10)
            where = rng.random(length) < d
            copy[where] = (copy[where] + 1 + rng.integers(0, 3, where.sum())) \
                % 4
            at = int(slots[f * members + k]) * (length + 64)
            text[at:at + length] = copy
    return text


def measure(name, index, text, seeds, L, K, S, queries, hostqueries,
            search_ms, stream):
    best = None
    for _ in range(3):
        res = V.extend_hamming(index, queries, seeds, L, K, S)
        st = res.stats()
        if best is None or st.search_kernel_ms < best[1].search_kernel_ms:
            best = (res, st)
    res, st = best
    got = res.fetch()
    nseeds = seeds.count
    t0 = time.time()
    hostseeds = seeds.fetch()
    t1 = time.time()
    host = V.extend_hamming_host(text, hostseeds, L, K, S,
                                 queries=hostqueries, threads=HOST_THREADS)
    t2 = time.time()
    same = bool(np.array_equal(got, host))
    # bytes the stages move at least, from the lists: per seed its record
    # twice (scan, choice), two entries of each look table written and read,
    # the two counts, the flag and the record of the choice; per match its
    # record once more and, in both texts, the symbols between the seed and
    # the ends of the match
    seedlen = int(hostseeds["length"].sum())
    ext = int(V.hamming_lengths(got).sum()) - \
        (seedlen * len(got) // max(1, nseeds))
    atleast = nseeds * (2 * 32 + 2 * 2 * 2 * 4 + 2 * 2 * 4 + 1 + 32) + \
        len(got) * 32 + 2 * max(0, ext)
    out = dict(
        workload=name, leastlength=L, maxdist=K,
        seedlength=V.extend_seedlength(L, K, S), seeds=nseeds,
        matches=int(st.count), long_sides=int(st.searches),
        long_share_of_sides=st.searches / (2.0 * max(1, nseeds)),
        seed_search_ms=search_ms, extension_ms=st.search_kernel_ms,
        scan_stage_ms=st.first_kernel_ms, long_stage_ms=st.anchor_ms,
        choice_stage_ms=st.search_kernel_ms - st.first_kernel_ms -
        st.anchor_ms,
        call_device_ms=st.total_device_ms,
        bytes_per_seed_atleast=atleast / max(1, nseeds),
        stream_read_gbps=stream,
        fraction_of_stream_read=(atleast / 1e9) /
        (st.search_kernel_ms / 1e3) / stream if st.search_kernel_ms > 0
        else None,
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
    ap.add_argument("--subst", type=int, default=3)
    ap.add_argument("--only", choices=("reads", "self"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18",
                                                  "extend_probe.json"))
    a = ap.parse_args()
    n, nq, m = int(a.n), int(a.nq), a.m
    rng = np.random.default_rng(18)
    stream = V.measure_stream_read()
    results = []
    if a.only != "self":
        genome = V.synth_genome(n)
        index = V.Index.build(genome, 4, 0, 0)
        reads = substituted_reads(rng, genome, nq, m, a.subst)
        dq = V.device_malloc(nq * m + 64)
        V.device_upload(dq, reads)
        queries = V.Queries.from_device(dq, nq, m)
        L, K, S = 100, 3, 0
        V.findquerymatches(index, queries, V.extend_seedlength(L, K, S)).close()
        V.device_synchronize()
        t0 = time.time()
        seeds = V.findquerymatches(index, queries,
                                   V.extend_seedlength(L, K, S))
        search_ms = (time.time() - t0) * 1e3
        hostq = (reads, np.arange(nq, dtype=np.uint64) * np.uint64(m),
                 np.full(nq, m, np.uint64))
        results.append(measure("reads", index, genome, seeds, L, K, S,
                               queries, hostq, search_ms, stream))
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
                               None, search_ms, stream))
        seeds.close()
        index.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(n=n, nq=nq, m=m, subst=a.subst, results=results), f,
                  indent=1)


if __name__ == "__main__":
    main()
