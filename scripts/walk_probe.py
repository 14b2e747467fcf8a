#!/usr/bin/env python3
"""The walk of the planned MUM search (mum_walk.inc) where it pays and where
it cannot: -mum -l 20, 100 bp reads against a 300 Mbp index,

  random   reads from the text with one substitution each: behind it l - 1
           offsets whose matches stop after about log4 n symbols -- the walk
           skips most of them
  repeat   reads with six substitutions from a window of the text that holds
           COPIES copies of one 2 kbp unit: the plan runs out of slots and
           stretches its last range over offsets that match to the end of the
           read in every copy; nothing there can be skipped, a lane locates
           every offset of its chunk one after the other
           (the whole text is not made of the unit: the index builder's lcp
           kernel starts every chunk of text positions from lcp 0 and would
           compare n symbols per chunk on a text of one period)

each with the walk off (VSA_TUNE=16, first and last) and with chunks of 4, 8
and 32 offsets, through the tile queue and (VSA_TUNE=32) through the workgroup
tiles: ms per call and kernel_searches.

  walk_probe.py [n [reads [calls]]]        all runs, one process each
  walk_probe.py --one KIND [n reads calls] one run under the environment given

Every run is a process of its own under a time limit of its own (the switches
are read when an index is created); the first one that fails ends the probe."""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, L, UNIT, COPIES = 100, 20, 2000, 100


def one(kind, n, nq, calls):
    sys.path.insert(0, ROOT)
    import vstree_amd as V
    rng = np.random.default_rng(13)
    tis = V.synth_genome(n)
    if kind == "repeat":
        w0 = n // 3
        tis[w0:w0 + UNIT * COPIES] = np.tile(
            rng.integers(0, 4, UNIT).astype(np.uint8), COPIES)
        pos = w0 + rng.integers(0, UNIT * COPIES - M, nq)
        places = np.sort(rng.integers(0, M // 6, (nq, 6)) +
                         np.arange(6) * (M // 6), axis=1)
    else:
        pos = rng.integers(0, n - M, nq)
        places = rng.integers(0, M, (nq, 1))
    reads = tis[pos[:, None] + np.arange(M)[None, :]]
    rows = np.arange(nq)[:, None]
    reads[rows, places] = (reads[rows, places] + 1 +
                           rng.integers(0, 3, places.shape)) & 3
    idx = V.Index.build(tis, 4, 0)
    q = V.Queries.from_host_packed(np.ascontiguousarray(reads).ravel(), M)
    r = V.findquerymatches(idx, q, L, mum=True)
    s = r.stats()
    r.close()
    best = None
    for rnd in range(3):
        V.device_synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            V.findquerymatches(idx, q, L, mum=True).close()
        V.device_synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / calls
        best = ms if best is None else min(best, ms)
    print("%-6s VSA_TUNE=%-2s VSA_WALK_CHUNK=%-2s  %.3f ms per call (best of 3 "
          "rounds of %d), kernel_searches %d, search kernel %.3f ms, "
          "candidates %d, MUMs %d" %
          (kind, os.environ.get("VSA_TUNE", "-"),
           os.environ.get("VSA_WALK_CHUNK", "-"), best, calls,
           s.kernel_searches, s.search_kernel_ms, s.candidates, s.count),
          flush=True)


def main():
    args = sys.argv[1:]
    if args[:1] == ["--one"]:
        kind = args[1]
        n, nq, calls = (int(float(x)) for x in args[2:5])
        one(kind, n, nq, calls)
        return 0
    vals = [int(float(x)) for x in args]
    n, nq, calls = vals + [300_000_000, 1_000_000, 20][len(vals):]
    for kind in ("random", "repeat"):
        # (VSA_TUNE=32: the workgroup tiles of k_query_search_planned instead
        # of the tile queue, the same chunks)
        for tune, chunk in (("16", None), (None, "4"), ("32", "4"),
                            (None, "8"), ("32", "8"), (None, "32"),
                            ("32", "32"), ("16", None)):
            env = dict(os.environ)
            env.pop("VSA_TUNE", None)
            env.pop("VSA_WALK_CHUNK", None)
            if tune is not None:
                env["VSA_TUNE"] = tune
            if chunk is not None:
                env["VSA_WALK_CHUNK"] = chunk
            try:
                rc = subprocess.run(
                    [sys.executable, os.path.abspath(__file__), "--one", kind,
                     str(n), str(nq), str(calls)], env=env,
                    timeout=240).returncode
            except subprocess.TimeoutExpired:
                print("walk_probe: %s timed out, stopping" % kind, flush=True)
                return 124
            if rc != 0:
                print("walk_probe: %s ended with %d, stopping" % (kind, rc),
                      flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
