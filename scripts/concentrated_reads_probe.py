#!/usr/bin/env python3
"""-mum -l 20 on reads that all come from ONE window of the text (amplicon
reads, a repeat family): the batch bench.py cannot make.  Their candidates
fall into one or two buckets of the candidate sort (candidate_sort.inc), a
bucket overflows, and the call falls back to compaction and rocPRIM's radix
sort -- this probe says what that detour costs.

  concentrated_reads_probe.py [--root TREE] [n [reads [window [calls]]]]

A 300 Mbp index, 1 M reads of 100 bp from a 1 Mbp window, 50 calls between two
device synchronisations, three rounds; --root: the tree whose library is
loaded (to run the same probe on another build)."""
import os
import sys
import time

import numpy as np

args = sys.argv[1:]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
given = args[:1] == ["--root"]
if given:
    ROOT = os.path.abspath(args[1])
    args = args[2:]
sys.path.insert(0, ROOT)
import vstree_amd as V  # noqa: E402

vals = [int(float(x)) for x in args]
n, nq, window, calls = (vals + [300_000_000, 1_000_000, 1_000_000, 50][len(vals):])
m, L = 100, 20
dg = V.device_malloc(n + 64)
V._check(V.lib.vsa_synth_genome_device(V.GENOME_SEED, n, dg, 0))
pos, sub, step = V.synth_query_plan(n, nq, m)
pos[:] = n // 3 + np.random.default_rng(5).integers(0, window - m, nq)
dq = V.device_malloc(nq * m + 64)
V._check(V.lib.vsa_synth_queries_device(dg, n, pos.ctypes.data,
                                        sub.ctypes.data, step.ctypes.data,
                                        nq, m, dq, 0))
q = V.Queries.from_device(dq, nq, m)
idx = V.Index.build_device(dg, n, 4, 0)
r = V.findquerymatches(idx, q, L, mum=True)
s = r.stats()
print("library of %s\n%d reads from a window of %d of %d positions: %d "
      "candidates, %d MUMs" % ("the tree given by --root" if given else
                               "this tree", nq, window, n, s.candidates,
                               s.count), flush=True)
r.close()


def counters(when):
    if hasattr(V.lib, "vsa_debug_candidate_sort"):
        import ctypes as C
        out = (C.c_uint64 * 5)()
        V.lib.vsa_debug_candidate_sort(out)
        print("%s: bucket sorts %d, of them overflowed %d (shift %d, %d "
              "buckets)" % (when, out[0], out[1], out[3], out[4]), flush=True)


counters("after the first call")
for rnd in range(3):
    V.device_synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        V.findquerymatches(idx, q, L, mum=True).close()
    V.device_synchronize()
    print("round %d: %.3f ms per call over %d calls" %
          (rnd, (time.perf_counter() - t0) * 1e3 / calls, calls), flush=True)
    counters("after round %d" % rnd)
