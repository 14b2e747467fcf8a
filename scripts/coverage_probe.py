#!/usr/bin/env python3
"""Match coverage on the headline workload: what mark, extract and count cost
on the device, next to what a caller has to do without them -- fetch the
match list and restate marksinglematch (Vmatch/markmat.c:30-40) on the host.

usage: coverage_probe.py [N [NQ [M [L]]]] [--repeats N2] [--out FILE]
  N, NQ, M, L  synthetic index of N bp, NQ reads of M bp, vmatch -l L
               (default 3e9, 1e7, 100, 20: the workload of bench.py)
  --repeats    length of the contended case: vsa_findmaximalrepeats on a text
               and its copy with one substitution every 97 bp (the text of
               bench.py --mode selfmum; default 2e7)
Prints one JSON line per list (and appends it to FILE): HIP-event times of
mark with and without the read before the atomic (VSA_COVERAGE_READFIRST),
of the extraction and of the count, for the database and the query side; the
bytes each kernel moves at least; the time of vsa_result_fetch plus the host
loop.  Every device table is compared with the host loop's.
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


def host_mark(nbits, seppos, starts, lengths):
    """marksinglematch for every instance, vectorised: +1 / -1 at the ends,
    running sum -> one byte per position, packed"""
    d = np.zeros(nbits + 1, np.int32)
    np.add.at(d, starts, 1)
    np.add.at(d, starts + lengths, -1)
    marked = np.cumsum(d[:-1]) > 0
    marked[seppos] = True
    pad = np.zeros((nbits + 63) // 64 * 64, bool)
    pad[:nbits] = marked
    return np.packbits(pad, bitorder="little").view(np.uint64)


def best(fn, reps=3):
    out = []
    for _ in range(reps):
        out.append(fn())
    return min(out)


def measure(cov_factory, result, kw, host_instances, nbits, seppos):
    """-> dict of times for one list and one side"""
    res = {}
    for readfirst in ("1", "0"):
        os.environ["VSA_COVERAGE_READFIRST"] = readfirst
        times = []
        for _ in range(3):
            cov = cov_factory()
            cov.mark(result, **kw)
            times.append(cov.stats().mark_ms)
            if _ < 2:
                cov.close()
        res["mark_ms" if readfirst == "1" else "mark_noread_ms"] = min(times)
    os.environ.pop("VSA_COVERAGE_READFIRST")
    ext = []
    for _ in range(3):
        iv = cov.nomatch(1)
        ext.append(cov.stats().extract_ms)
    res["extract_ms"], res["runs"] = min(ext), len(iv)
    res["count_ms"] = best(lambda: cov.stats().count_ms)
    st = cov.stats()
    res["positions"], res["marked"] = st.positions, st.marked
    # what a caller does today
    t0 = time.time()
    m = result.fetch()
    res["fetch_ms"] = (time.time() - t0) * 1e3
    t0 = time.time()
    starts, lengths = host_instances(m)
    words = host_mark(nbits, seppos, starts, lengths)
    res["host_mark_ms"] = (time.time() - t0) * 1e3
    assert np.array_equal(words, cov.bits()), "device table != host table"
    # least traffic: the records once, the table once per pass over it
    res["mark_bytes"] = 32 * len(m)
    res["table_bytes"] = (nbits + 63) // 64 * 8
    cov.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="?", type=float, default=3e9)
    ap.add_argument("nq", nargs="?", type=float, default=1e7)
    ap.add_argument("m", nargs="?", type=int, default=100)
    ap.add_argument("L", nargs="?", type=int, default=20)
    ap.add_argument("--repeats", type=float, default=2e7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, nq, m, L = int(a.n), int(a.nq), a.m, a.L
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    if n > 0:
        dg = V.device_malloc(n + 64)
        V._check(V.lib.vsa_synth_genome_device(V.GENOME_SEED, n, dg, 0))
        index = V.Index.build_device(dg, n, 4, 0)
        pos, sub, step = V.synth_query_plan(n, nq, m)
        dq = V.device_malloc(nq * m + 64)
        V._check(V.lib.vsa_synth_queries_device(
            dg, n, pos.ctypes.data, sub.ctypes.data, step.ctypes.data, nq, m,
            dq, 0))
        queries = V.Queries.from_device(dq, nq, m)
        qsep = (np.arange(1, nq, dtype=np.int64) * (m + 1)) - 1
        for name, kw in (("mum", dict(mum=True)), ("mem", {})):
            r = V.findquerymatches(index, queries, L, **kw)
            for side in ("database", "queries"):
                if side == "database":
                    d = measure(
                        lambda: V.Coverage.over_index(index), r,
                        dict(layout=V.COVERAGE_QUERY,
                             side=V.COVERAGE_DATABASE),
                        lambda x: (x["dbstart"].astype(np.int64),
                                   x["length"].astype(np.int64)),
                        n, np.zeros(0, np.int64))
                else:
                    d = measure(
                        lambda: V.Coverage.over_queries(queries), r,
                        dict(layout=V.COVERAGE_QUERY,
                             side=V.COVERAGE_QUERIES),
                        lambda x: ((x["queryseq"] * np.uint64(m + 1) +
                                    x["querystart"]).astype(np.int64),
                                   x["length"].astype(np.int64)),
                        nq * (m + 1) - 1, qsep)
                d.update(list="-%s -l %d" % (name, L) if name == "mum"
                         else "-l %d" % L, side=side, n=n, nq=nq, m=m,
                         matches=r.count)
                emit(d)
            r.close()
        index.close()
    if a.repeats > 0:
        n2 = int(a.repeats)
        half = (n2 - 1) // 2
        g = V.synth_genome(half)
        g2 = g.copy()
        g2[::97] = (g2[::97] + 1) & 3
        tis = np.concatenate([g, np.array([255], np.uint8), g2])
        index = V.Index.build(tis, 4, 0)
        r = V.findmaximalrepeats(index, L)

        def both(x):
            return (np.concatenate([x["dbstart"], x["queryseq"]]).astype(
                np.int64), np.concatenate([x["length"], x["length"]]).astype(
                    np.int64))
        d = measure(lambda: V.Coverage.over_index(index), r,
                    dict(layout=V.COVERAGE_SELF, side=V.COVERAGE_DATABASE),
                    both, len(tis), np.array([half], np.int64))
        d.update(list="maximal repeats -l %d" % L, side="database",
                 n=len(tis), matches=r.count)
        emit(d)
    if a.out:
        with open(a.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
