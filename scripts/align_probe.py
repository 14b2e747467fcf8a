#!/usr/bin/env python3
"""The alignment of degenerate matches (vmatch -s: vsa_align) on the two match
lists of scripts/extend_edist_probe.py, next to what a caller has to do
without it -- the fetch of the match list plus vsa_align_host on 16 threads,
timed in the same run:

  reads  the matches of NQ reads of M symbols (substitutions, and one insertion
         or deletion in every second read) against a random index of N
         symbols, -l 60 -e 3 -q
  self   the matches of a random text of N symbols with planted repeat families
         against itself, -l 100 -e 5 -seedlength 20

usage: align_probe.py [N [NQ [M]]] [--only reads|self] [--out FILE]
       (default 1e8, 1e7, 150; FILE default profiles/r23/align_probe.json)

Per workload one JSON object: matches, words of all scripts, the records whose
group finished a slide together, the HIP-event times of vsa_align (the median
of REPEAT calls after one that is not timed: the two alignment kernels, and the
whole call with count, scans and gather), the wall time of the fetch of the
scripts, the algorithmic bytes (both substrings read about twice, the script
written), and the host figures.  The device scripts are compared with the
host's.
"""
import argparse
import json
import os
import statistics
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
REPEAT = 5


def measure(name, index, text, matches, kind, queries, hostqueries):
    V.align(index, queries, matches, kind).close()
    V.device_synchronize()
    kernel, call = [], []
    al = None
    for _ in range(REPEAT):
        if al is not None:
            al.close()
        al = V.align(index, queries, matches, kind)
        st = al.stats()
        kernel.append(st.kernel_ms)
        call.append(st.total_device_ms)
    t0 = time.time()
    offsets, words = al.fetch()
    t1 = time.time()
    rec = matches.fetch()
    t2 = time.time()
    host = V.align_host(kind, text, rec, hostqueries, threads=HOST_THREADS)
    t3 = time.time()
    same = bool(np.array_equal(offsets, host[0]) and
                np.array_equal(words, host[1]))
    symbols = int(V.edist_lengths1(rec).sum() + V.edist_lengths2(rec).sum())
    out = dict(
        workload=name, matches=int(st.count), words=int(st.words),
        aligned_by_fronts=int(st.edist), group_finished_slides=int(st.staged),
        largest_distance=int(V.edist_distances(rec).max()) if len(rec) else 0,
        repetitions=REPEAT, warm_calls=1,
        align_kernels_ms=statistics.median(kernel),
        align_kernels_ms_all=kernel,
        align_call_device_ms=statistics.median(call),
        align_call_device_ms_all=call,
        script_fetch_ms=(t1 - t0) * 1e3,
        algorithmic_bytes=2 * symbols + 2 * int(st.words) + 32 * len(rec),
        host_threads=HOST_THREADS, list_fetch_ms=(t2 - t1) * 1e3,
        host_align_ms=(t3 - t2) * 1e3,
        fetch_plus_host_ms=(t3 - t1) * 1e3, device_equals_host=same)
    print(json.dumps(out), flush=True)
    al.close()
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
        ROOT, "profiles", "r23", "align_probe.json"))
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
        print("reads: index and batch are there", flush=True)
        matches = V.findquerymatches_edist(index, queries, 60, 3)
        print("reads: %d matches" % matches.count, flush=True)
        hostq = (reads, np.arange(nq, dtype=np.uint64) * np.uint64(m),
                 np.full(nq, m, np.uint64))
        results.append(measure("reads", index, genome, matches,
                               V.SINK_QUERY_EDIST, queries, hostq))
        matches.close()
        queries.close()
        V.device_free(dq)
        index.close()
    if a.only != "reads":
        text = planted_text(rng, n, max(1, n // 50000), 6, 2000)
        index = V.Index.build(text, 4, 0, 0)
        print("self: the index is there", flush=True)
        matches = V.findselfmatches_edist(index, 100, 5, 20)
        print("self: %d matches" % matches.count, flush=True)
        results.append(measure("self", index, text, matches,
                               V.SINK_SELF_EDIST, None, None))
        matches.close()
        index.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(n=n, nq=nq, m=m, subst=a.subst, results=results), f,
                  indent=1)


if __name__ == "__main__":
    main()
