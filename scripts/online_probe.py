#!/usr/bin/env python3
"""Times the scan without an index (vmatch -online -complete) on a
synthetic text: for m = 100 and 1, 64 and 4096 queries, -e 2, -e 5, -h 3 and
exact through

  * the device entry on a vsa_text: the HIP-event times of its stats (whole
    call, both scans, the first pass alone), best of five after a warm-up;
    symbol-steps per second (text symbols x queries / time of the scans)
    against the first-order figure of DESIGN 4k, and the share of the second
    pass;
  * vsa_findcompletematches_online_host on 16 threads (--host-queries of
    the batch, scaled);
  * with --indexed: vsa_findapproxcompletematches / vsa_findcompletematches
    on an index of the same text built on the GPU;
  * with --reference: the real `vmatch -online` of oracle/_ref on one query;
  * -e 2 remred on a text of tandems of period 2 (the remred stage walks a
    run of start positions with one lane).

    python3 scripts/online_probe.py [--n 3000000000] [--out DIR]

Writes online_probe.json into DIR (default: the next round directory under
profiles/).  No number here is a pass or fail bar.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import vstree_amd as V  # noqa: E402

CONFIGS = (("e2", V.ONLINE_EDIST, 2), ("e5", V.ONLINE_EDIST, 5),
           ("h3", V.ONLINE_HAMMING, 3), ("exact", V.ONLINE_EXACT, 0))
LANE_INSTRUCTIONS = 256 * 4 * 16 * 2.4e9   # DESIGN 4k, first order


def next_round():
    base = os.path.join(ROOT, "profiles")
    have = [int(d[1:]) for d in os.listdir(base)
            if d[0] == "r" and d[1:].isdigit()]
    return os.path.join(base, "r%02d" % (max(have) + 1))


def best_of(call, reps=5):
    call().close()                                   # warm-up
    best = None
    for _ in range(reps):
        r = call()
        s = r.stats().asdict()
        s["count"] = r.count
        r.close()
        if best is None or s["total_device_ms"] < best["total_device_ms"]:
            best = s
    return best


def device_rows(text, n, g, m, counts, remred=False, configs=CONFIGS):
    rows = []
    for nq in counts:
        qb = V.synth_queries(g, nq, m)
        gq = V.Queries.from_host(qb, np.arange(nq, dtype=np.uint64) * m,
                                 np.full(nq, m, np.uint64))
        for name, mode, k in configs:
            s = best_of(lambda: V.findcompletematches_online(
                text, gq, mode, k, False, remred))
            scan = s["search_kernel_ms"]
            rows.append(dict(
                config=name + ("_remred" if remred else ""), queries=nq,
                matches=s["count"], startpositions=s["candidates"],
                pairs_second_pass=s["searches"],
                total_device_ms=s["total_device_ms"], scans_ms=scan,
                first_pass_ms=s["first_kernel_ms"],
                second_pass_share=(scan - s["first_kernel_ms"]) / scan
                if scan > 0 else 0.0,
                symbol_steps_per_s=n * nq / (scan * 1e-3) if scan > 0 else 0,
                lane_instruction_figure=LANE_INSTRUCTIONS))
            print(rows[-1], flush=True)
        gq.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3000000000)
    ap.add_argument("--m", type=int, default=100)
    ap.add_argument("--queries", default="1,64,4096")
    ap.add_argument("--host-queries", type=int, default=2)
    ap.add_argument("--indexed", action="store_true")
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = a.out or next_round()
    os.makedirs(out, exist_ok=True)
    n, m = a.n, a.m
    counts = [int(x) for x in a.queries.split(",")]
    g = V.synth_genome(n)
    text = V.Text.from_host(g)
    res = dict(n=n, m=m, device=device_rows(text, n, g, m, counts))
    # the host entry, a few queries on 16 threads
    hq = V.synth_queries(g, a.host_queries, m)
    res["host"] = []
    for name, mode, k in CONFIGS:
        t0 = time.time()
        got = V.findcompletematches_online_host(
            g, hq, np.arange(a.host_queries, dtype=np.uint64) * m,
            np.full(a.host_queries, m, np.uint64), mode, k, threads=16)
        dt = time.time() - t0
        res["host"].append(dict(config=name, queries=a.host_queries,
                                threads=16, seconds=dt, matches=len(got),
                                seconds_per_query=dt / a.host_queries))
        print(res["host"][-1], flush=True)
    if a.indexed:
        index = V.Index.build(g, 4, 0, 0)
        res["indexed"] = []
        for nq in counts:
            qb = V.synth_queries(g, nq, m)
            gq = V.Queries.from_host(qb, np.arange(nq, dtype=np.uint64) * m,
                                     np.full(nq, m, np.uint64))
            for name, mode, k in CONFIGS:
                call = (lambda: V.findcompletematches(index, gq)) \
                    if mode == V.ONLINE_EXACT else \
                    (lambda: V.findapproxcompletematches(
                        index, gq, mode == V.ONLINE_EDIST, k))
                s = best_of(call)
                res["indexed"].append(dict(
                    config=name, queries=nq, matches=s["count"],
                    total_device_ms=s["total_device_ms"]))
                print(res["indexed"][-1], flush=True)
            gq.close()
        index.close()
    text.close()
    if a.reference:
        import helpers as H
        wd = tempfile.mkdtemp()
        chars = np.frombuffer(b"acgt", np.uint8)
        H.write_fasta_fast(wd + "/db.fna", [("g", chars[g].tobytes())])
        with open(wd + "/q.fna", "w") as f:
            f.write(">q\n%s\n" % chars[hq[:m]].tobytes().decode())
        H.run_mkvtree_ref(["-indexname", "db.fna", "-db", "db.fna", "-dna",
                           "-pl", "-tis", "-ois"], wd)
        res["reference"] = []
        for name, mode, k in CONFIGS:
            args = ["-online", "-complete"] + \
                ([] if mode == V.ONLINE_EXACT else
                 ["-e" if mode == V.ONLINE_EDIST else "-h", str(k)])
            t0 = time.time()
            subprocess.run([H.VMATCH_REF] + args + ["-q", "q.fna", "db.fna"],
                           cwd=wd, stdout=subprocess.DEVNULL, check=True)
            res["reference"].append(dict(config=name, queries=1,
                                         seconds=time.time() - t0))
            print(res["reference"][-1], flush=True)
        shutil.rmtree(wd)
    # remred on tandems: runs of start positions as long as a region
    tn = min(n, 1 << 24)
    tg = np.tile(np.array([0, 3], np.uint8), tn // 2)
    tg[::100003] = 1
    ttext = V.Text.from_host(tg)
    rq = np.tile(np.array([0, 3], np.uint8), m // 2)
    gq = V.Queries.from_host(rq, [0], [len(rq)])
    res["remred_tandem"] = []
    for remred in (False, True):
        t0 = time.time()
        r = V.findcompletematches_online(ttext, gq, V.ONLINE_EDIST, 2, False,
                                         remred)
        res["remred_tandem"].append(dict(
            n=tn, remred=remred, matches=r.count, wall_s=time.time() - t0,
            total_device_ms=r.stats().total_device_ms))
        print(res["remred_tandem"][-1], flush=True)
        r.close()
    with open(os.path.join(out, "online_probe.json"), "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", os.path.join(out, "online_probe.json"))


if __name__ == "__main__":
    main()
