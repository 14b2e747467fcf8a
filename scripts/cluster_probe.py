#!/usr/bin/env python3
"""Sequence clustering at the order of magnitude of the headline's match
list: what vsa_cluster_add, vsa_cluster_finish and vsa_cluster_edges cost on
the device, next to what a caller has to do without them -- vsa_result_fetch
of the whole list plus the same rules on the host (vsa_cluster_host).

usage: cluster_probe.py [RECORDS [SEQUENCES [FAMILY]]] [--out FILE]
  A synthetic self list of RECORDS matches (default 1e7) over SEQUENCES
  sequences of 100 symbols (default 2^20), EST style: both sequences of a
  match come from one family of FAMILY neighbouring sequences (default 256),
  one match in twenty lies inside one sequence, the lengths are 30..100 and
  -dbcluster 50 50 accepts those of 50 and more.  Needs no reference program.
Prints one JSON line (and writes it to FILE): per call the HIP-event time of
its kernels and copies (vsa_cluster_times) and the wall time with the host's
part (the replay of the forest, the waits), minimum and median of REPEATS
runs after one warm-up run; the rounds of the forest search; the fetch and
the host clustering.  The device's answer is compared with the host's.
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
import vstree_amd as V  # noqa: E402

SEQLEN = 100
REPEATS = 5


def synthetic_list(nrec, nseq, family, seed=7):
    rng = np.random.default_rng(seed)
    rec = np.zeros(nrec, V.MATCH_DTYPE)
    fam = rng.integers(0, nseq // family, nrec) * family
    s1 = fam + rng.integers(0, family, nrec)
    s2 = fam + rng.integers(0, family, nrec)
    inside = rng.integers(0, 20, nrec) == 0
    s2[inside] = s1[inside]
    lo, hi = np.minimum(s1, s2), np.maximum(s1, s2)
    rec["length"] = rng.integers(30, SEQLEN + 1, nrec)
    room = SEQLEN - rec["length"].astype(np.int64)
    rec["dbstart"] = lo * (SEQLEN + 1) + rng.integers(0, SEQLEN, nrec) % (
        room + 1)
    rec["queryseq"] = hi * (SEQLEN + 1) + rng.integers(0, SEQLEN, nrec) % (
        room + 1)
    return rec


def both(values):
    return dict(min=round(min(values), 3),
                median=round(statistics.median(values), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("records", nargs="?", type=float, default=1e7)
    ap.add_argument("sequences", nargs="?", type=float, default=2 ** 20)
    ap.add_argument("family", nargs="?", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nrec, nseq, family = int(a.records), int(a.sequences), a.family
    if V.device_count() < 1:
        sys.exit("cluster_probe.py needs a GPU")
    rec = synthetic_list(nrec, nseq, family)
    total = nseq * (SEQLEN + 1) - 1
    markpos = np.arange(1, nseq, dtype=np.uint64) * np.uint64(SEQLEN + 1) - \
        np.uint64(1)
    layout = V.sink_params(kind=V.SINK_SELF, totallength=total,
                           markpos=markpos)
    res = V.Result.from_host(rec)
    ev = {k: [] for k in ("add", "finish", "edges")}
    wall = {k: [] for k in ("add", "finish", "edges")}
    fetch, hostms = [], []
    for run in range(REPEATS + 1):
        cl = V.Cluster(layout, 50, 50)
        V.device_synchronize()
        t0 = time.perf_counter()
        cl.add(res)
        t1 = time.perf_counter()
        cl.finish()
        t2 = time.perf_counter()
        edges, eflags, estart = cl.edges()
        t3 = time.perf_counter()
        if run > 0:                              # run 0 warms up
            for k, v in zip(("add", "finish", "edges"), cl.times()):
                ev[k].append(v)
            wall["add"].append((t1 - t0) * 1e3)
            wall["finish"].append((t2 - t1) * 1e3)
            wall["edges"].append((t3 - t2) * 1e3)
        st = cl.stats()
        start, members = cl.members()
        labels = cl.labels()
        grouped = edges.fetch()
        edges.close()
        cl.close()
        # what a caller does today: the whole list over PCIe and the same
        # rules there
        t0 = time.perf_counter()
        host = res.fetch()
        t1 = time.perf_counter()
        want = V.cluster_host(layout, 50, 50, host, text=False)
        t2 = time.perf_counter()
        if run > 0:
            fetch.append((t1 - t0) * 1e3)
            hostms.append((t2 - t1) * 1e3)
    hst = want["stats"].asdict()
    dst = st.asdict()
    rounds = dst.pop("rounds")
    hst.pop("rounds")
    assert dst == hst, (dst, hst)
    assert np.array_equal(start, want["clusterstart"])
    assert np.array_equal(members, want["members"])
    assert np.array_equal(labels, want["labels"])
    assert np.array_equal(estart, want["edgestart"])
    assert np.array_equal(grouped,
                          host[want["edgerecord"].astype(np.int64)])
    device = [x + y + z for x, y, z in zip(wall["add"], wall["finish"],
                                           wall["edges"])]
    parent = [x + y for x, y in zip(fetch, hostms)]
    d = dict(records=nrec, sequences=nseq, family=family, seqlen=SEQLEN,
             percsmall=50, perclarge=50, repeats=REPEATS, stats=dst,
             rounds=rounds,
             event_ms={k: both(v) for k, v in ev.items()},
             wall_ms={k: both(v) for k, v in wall.items()},
             device_wall_ms=both(device),
             members_only_wall_ms=both([x + y for x, y in zip(
                 wall["add"], wall["finish"])]),
             fetch_ms=both(fetch), fetch_bytes=32 * nrec,
             host_cluster_ms=both(hostms), parent_ms=both(parent),
             ratio_parent_over_device=round(
                 statistics.median(parent) / statistics.median(device), 2),
             equal_to_host=True)
    print(json.dumps(d), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
