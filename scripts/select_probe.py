#!/usr/bin/env python3
"""Match selection on the headline workload: what -best 50, -best 10^6 and
-evalue alone cost on the device, next to what a caller has to do without
them -- vsa_result_fetch of the whole list plus the same rules on the host
(vsa_select_host).

usage: select_probe.py [N [NQ [M [L]]]] [--out FILE]
  N, NQ, M, L  synthetic index of N bp, NQ reads of M bp, the MUM candidates
               of vmatch -mum cand -l L (default 3e9, 1e7, 100, 20: the
               workload of bench.py)
Prints one JSON line per selection (and appends it to FILE): wall time of
vsa_select_add and vsa_select_finish (both wait for the device), the
digit-counting passes of the radix select, the bytes the kernels move at
least, the time of the fetch and of the host selection.  Every selection of
the device is compared with the host's.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="?", type=float, default=3e9)
    ap.add_argument("nq", nargs="?", type=float, default=1e7)
    ap.add_argument("m", nargs="?", type=int, default=100)
    ap.add_argument("L", nargs="?", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, nq, m, L = int(a.n), int(a.nq), a.m, a.L
    dg = V.device_malloc(n + 64)
    V._check(V.lib.vsa_synth_genome_device(V.GENOME_SEED, n, dg, 0))
    index = V.Index.build_device(dg, n, 4, 0)
    pos, sub, step = V.synth_query_plan(n, nq, m)
    dq = V.device_malloc(nq * m + 64)
    V._check(V.lib.vsa_synth_queries_device(
        dg, n, pos.ctypes.data, sub.ctypes.data, step.ctypes.data, nq, m,
        dq, 0))
    queries = V.Queries.from_device(dq, nq, m)
    r = V.findquerymatches(index, queries, L, mum=True, cand=True)
    count = r.count
    qlen = np.full(nq, m, np.uint64)
    qstart = np.arange(nq, dtype=np.uint64) * np.uint64(m + 1)
    layout = V.sink_params(kind=V.SINK_QUERY, totallength=n, markpos=[],
                           querystart=qstart, querylength=qlen,
                           querytotallength=nq * (m + 1) - 1, leastlength=L)
    # what a caller does today: the whole list over PCIe ...
    fetch = []
    for _ in range(3):
        t0 = time.time()
        host = r.fetch()
        fetch.append((time.time() - t0) * 1e3)
    lines = []
    for name, opts in (("-best 50", dict(best=50)),
                       ("-best 1000000", dict(best=10 ** 6)),
                       ("-evalue 1e-10", dict(evalue=1e-10))):
        add, fin, passes = [], [], 0
        for _ in range(3):
            sel = V.Select(layout, queries, **opts)
            V.device_synchronize()
            t0 = time.time()
            sel.add(r)
            t1 = time.time()
            out = sel.finish()
            t2 = time.time()
            add.append((t1 - t0) * 1e3)
            fin.append((t2 - t1) * 1e3)
            passes, st = sel.passes, sel.stats()
            got = out.fetch()
            sel.close()
        # ... and the same rules there
        t0 = time.time()
        want, _, _, hst = V.select_host(layout, host, **opts)
        host_ms = (time.time() - t0) * 1e3
        assert np.array_equal(got, want), name
        survivors = st.seen - st.rejected
        d = dict(selection=name, n=n, nq=nq, m=m, L=L, matches=count,
                 selected=len(got), rejected=st.rejected,
                 add_ms=min(add), finish_ms=min(fin),
                 device_ms=min(x + y for x, y in zip(add, fin)),
                 radix_passes=passes,
                 # the records twice (count, write), the five key words of
                 # every survivor once, one word of them per pass, the
                 # comparison with the threshold once
                 passes_over_list=2 + (passes + 1 if opts.get("best") else 0),
                 bytes_moved_at_least=64 * count + (
                     (40 + 8 * passes + 8) * survivors if opts.get("best")
                     else 33 * survivors),
                 fetch_ms=min(fetch), fetch_bytes=32 * count,
                 host_select_ms=host_ms,
                 parent_ms=min(fetch) + host_ms)
        print(json.dumps(d), flush=True)
        lines.append(d)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
