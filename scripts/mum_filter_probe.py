#!/usr/bin/env python3
"""The MUM filter on the paths bench.py does not take: candidate RECORDS
(vsa_mumuniqueinquery: composite keys + index, sorted on all bits), packed
PAIRS with a run of equal dbstarts that is too long for the filter by runs
(vsa_mumuniqueinquery_range_packed: sorted on dbstart, filtered, sorted on
all bits, filtered again), and WIDE records (the first list with dbstart +
2^40 and length + 2^30, which no key holds: the records sorted twice, the
filter on the sorted records).

  mum_filter_probe.py [--root TREE] [n]

n = 10 M synthetic candidates, every dbstart once, lengths from [20, 300);
the pairs carry one run of 200 on top.  One call to warm up, then
stats().total_device_ms of five calls each; --root: the tree whose library is
loaded (to run the same probe on another build)."""
import os
import sys

import numpy as np

args = sys.argv[1:]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
given = args[:1] == ["--root"]
if given:
    ROOT = os.path.abspath(args[1])
    args = args[2:]
sys.path.insert(0, ROOT)
import vstree_amd as V  # noqa: E402

n = int(float(args[0])) if args else 10_000_000
rng = np.random.default_rng(21)
cand = np.zeros(n, V.MATCH_DTYPE)
cand["dbstart"] = rng.permutation(3 * n)[:n]
cand["length"] = rng.integers(20, 300, n)
cand["queryseq"] = np.arange(n)
cand["querystart"] = rng.integers(0, 500, n)
print("library of %s, %d candidates" %
      ("the tree given by --root" if given else "this tree", n), flush=True)


def probe(name, call):
    times = []
    for i in range(6):
        r = call()
        s = r.stats()
        times.append(s.total_device_ms)
        r.close()
    print("%s: %d MUMs, sum of lengths %d; warm-up %.3f ms, then %s ms; "
          "median %.3f, max - min %.3f" %
          (name, s.count, s.sumlength, times[0],
           " ".join("%.3f" % t for t in times[1:]),
           float(np.median(times[1:])), max(times[1:]) - min(times[1:])),
          flush=True)


dp = V.device_malloc(cand.nbytes)
V.device_upload(dp, cand)
probe("records", lambda: V.mumuniqueinquery(dp, n))
wide = cand.copy()
wide["dbstart"] += np.uint64(1 << 40)
wide["length"] += np.uint64(1 << 30)


def widecall():
    V.device_upload(dp, wide)  # (the wide form sorts the records in place)
    return V.mumuniqueinquery(dp, n)


probe("wide records", widecall)
del wide
V.device_free(dp)

cand["dbstart"][:200] = 3 * n // 2
cand["length"][:200] = rng.permutation(np.arange(100, 300))
rows = np.zeros((n, 2), np.uint64)
rows[:, 0] = (cand["dbstart"] << np.uint64(9)) | (np.uint64(511) -
                                                  cand["length"])
rows[:, 1] = (cand["queryseq"] << np.uint64(16)) | cand["querystart"]
dp = V.device_malloc(rows.nbytes)
V.device_upload(dp, rows)
probe("pairs with a run of 200",
      lambda: V.mumuniqueinquery_range_packed(dp, n, 9, 3 * n + 300, 0))
V.device_free(dp)
