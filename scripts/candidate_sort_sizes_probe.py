#!/usr/bin/env python3
"""From how many candidates on does the bucket sort (candidate_sort.inc) beat
compaction + rocPRIM's radix sort?  -mum -l 20 on batches of growing size,
one index created under VSA_TUNE=4 (rocPRIM) and one under VSA_TUNE=8
(buckets): ms per call over 30 calls between two device synchronisations.
The answer is VSA_CS_MINPAIRS in esa_search.hip.

  candidate_sort_sizes_probe.py [n [largest batch]]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vstree_amd as V  # noqa: E402

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 300_000_000
top = int(float(sys.argv[2])) if len(sys.argv) > 2 else 4_000_000
m, L, calls = 100, 20, 30
dg = V.device_malloc(n + 64)
V._check(V.lib.vsa_synth_genome_device(V.GENOME_SEED, n, dg, 0))
idx = {}
for tune in (4, 8):
    os.environ["VSA_TUNE"] = str(tune)
    idx[tune] = V.Index.build_device(dg, n, 4, 0)
del os.environ["VSA_TUNE"]
nq = 16_384
while nq <= top:
    pos, sub, step = V.synth_query_plan(n, nq, m)
    dq = V.device_malloc(nq * m + 64)
    V._check(V.lib.vsa_synth_queries_device(dg, n, pos.ctypes.data,
                                            sub.ctypes.data, step.ctypes.data,
                                            nq, m, dq, 0))
    q = V.Queries.from_device(dq, nq, m)
    ms = {}
    for tune in (4, 8, 4, 8):
        r = V.findquerymatches(idx[tune], q, L, mum=True)
        cand = r.stats().candidates
        r.close()
        V.device_synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            V.findquerymatches(idx[tune], q, L, mum=True).close()
        V.device_synchronize()
        t = (time.perf_counter() - t0) * 1e3 / calls
        ms[tune] = min(ms.get(tune, t), t)
    print("%9d reads %9d candidates: rocPRIM %.3f ms  buckets %.3f ms per call"
          % (nq, cand, ms[4], ms[8]), flush=True)
    q.close()
    V.device_free(dq)
    nq *= 2
