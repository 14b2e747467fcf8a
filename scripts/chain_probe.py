#!/usr/bin/env python3
"""Chaining at the order of magnitude of the headline's match list: what
vsa_chain_add and _finish cost on the device, stage by stage (view, sort,
replay, score, retrieve), next to what a caller has to do without them --
vsa_result_fetch of the whole list plus vsa_chain_host.

usage: chain_probe.py [--records N] [--only reads|long|bound] [--kind K]
                      [--bounds SMALL,WAVE ...] [--out FILE]
Three synthetic lists against queries (withinborders: one chaining problem
per (database sequence, query) pair), without ties like a -mum list:
  reads  about N / 2.5 pairs of 1 to 6 fragments: reads of 150 bp against a
         text of 24 sequences; every problem takes the one-lane kernel
  long   pairs of 20 to 200 fragments: the wavefront and workgroup kernels
  bound  N / 2^15 problems of 2^15 fragments each, the most the device takes
--bounds runs a list again with other class boundaries (the environment
variables VSA_CHAIN_SMALLMAX and VSA_CHAIN_WAVEMAX of vsa_chain_finish): the
A/B behind the constants of chain_rules.h.  Prints one JSON line per case and
setting (and appends it to FILE): per stage the HIP-event time
(vsa_chain_times), per call the wall time, minimum and median of three runs
after one warm-up run; the fetch and the host chaining; the device's answer
is compared with the host's.  Needs no reference program.
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

NSEQ = 24


def both(values):
    return dict(min=round(min(values), 3),
                median=round(statistics.median(values), 3))


def make_list(sizes, step, seed):
    """one problem per query: query q has sizes[q] fragments of 15 symbols,
    `step` apart on the query, near a diagonal of the database sequence
    q % NSEQ -> (records, layout)"""
    rng = np.random.default_rng(seed)
    nq = len(sizes)
    n = int(sizes.sum())
    qlen = int(sizes.max()) * step + 40
    q = np.repeat(np.arange(nq, dtype=np.uint64), sizes)
    first = np.concatenate(([0], np.cumsum(sizes)[:-1]))
    k = np.arange(n, dtype=np.uint64) - np.repeat(first, sizes).astype(
        np.uint64)
    seqlen = 4 * qlen + 1000
    rec = np.zeros(n, V.MATCH_DTYPE)
    rec["length"] = 15
    rec["queryseq"] = q
    rec["querystart"] = k * np.uint64(step) + rng.integers(
        0, step - 15, n).astype(np.uint64)
    rec["dbstart"] = (q % np.uint64(NSEQ)) * np.uint64(seqlen + 1) + \
        rng.integers(0, 2 * qlen, nq).astype(np.uint64)[q.astype(np.int64)] \
        + k * np.uint64(step) + rng.integers(0, 2 * step, n).astype(np.uint64)
    rec = rec[rng.permutation(n)]
    layout = V.sink_params(
        kind=V.SINK_QUERY, totallength=NSEQ * (seqlen + 1) - 1,
        markpos=np.arange(1, NSEQ, dtype=np.uint64) * np.uint64(seqlen + 1) -
        np.uint64(1),
        querystart=np.arange(nq, dtype=np.uint64) * np.uint64(qlen + 1),
        querylength=np.full(nq, qlen, np.uint64),
        querytotallength=nq * (qlen + 1) - 1)
    return rec, layout


def cases(nrec):
    rng = np.random.default_rng(1)
    yield "reads", rng.choice(np.arange(1, 7), int(nrec / 2.5),
                              p=[.35, .25, .15, .1, .1, .05]), 22, 2
    yield "long", rng.integers(20, 201, int(nrec / 110)), 24, 3
    yield "bound", np.full(max(1, nrec >> 15), 1 << 15), 18, 4


def device_run(layout, res, opt):
    ch = V.Chain(layout, **opt)
    V.device_synchronize()
    t0 = time.perf_counter()
    ch.add(res)
    t1 = time.perf_counter()
    ch.finish()
    t2 = time.perf_counter()
    return ch, ((t1 - t0) * 1e3, (t2 - t1) * 1e3)


def measure(layout, res, opt, reps=3):
    device_run(layout, res, opt)[0].close()      # warm-up
    ev = {k: [] for k in V.CHAIN_STAGES}
    wall = dict(add=[], finish=[])
    for _ in range(reps):
        ch, (a, f) = device_run(layout, res, opt)
        for k, v in ch.times().items():
            ev[k].append(v)
        wall["add"].append(a)
        wall["finish"].append(f)
        last = ch
    return last, ev, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=float, default=1e7)
    ap.add_argument("--only", default=None)
    ap.add_argument("--kind", type=int, default=V.CHAIN_LOCAL_MAX)
    ap.add_argument("--bounds", action="append", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if V.device_count() < 1:
        sys.exit("chain_probe.py needs a GPU")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def report(d):
        print(json.dumps(d), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(d) + "\n")

    opt = dict(kind=a.kind, withinborders=True)
    for name, sizes, step, seed in cases(int(a.records)):
        if a.only and a.only != name:
            continue
        rec, layout = make_list(sizes.astype(np.int64), step, seed)
        res = V.Result.from_host(rec)
        ch, ev, wall = measure(layout, res, opt)
        st = ch.stats().asdict()
        got = ch.chains()
        ch.close()
        fetch = []
        for _ in range(3):
            t0 = time.perf_counter()
            host = res.fetch()
            fetch.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        want = V.chain_host(layout, host, **opt)
        hostms = (time.perf_counter() - t0) * 1e3 / 2   # it runs twice
        assert st == want["stats"].asdict(), (st, want["stats"].asdict())
        for k in ("problem", "number", "score", "start", "members"):
            assert np.array_equal(got[k], want[k]), k
        device = [x + y for x, y in zip(wall["add"], wall["finish"])]
        parent = statistics.median(fetch) + hostms
        report(dict(case=name, kind=a.kind, records=len(rec), stats=st,
                    bounds="8,64", event_ms={k: both(v)
                                             for k, v in ev.items()},
                    wall_ms={k: both(v) for k, v in wall.items()},
                    device_wall_ms=both(device), fetch_ms=both(fetch),
                    host_chain_ms=round(hostms, 3),
                    parent_ms=round(parent, 3),
                    ratio_parent_over_device=round(
                        parent / statistics.median(device), 2),
                    equal_to_host=True))
        for spec in a.bounds or []:
            small, wave = spec.split(",")
            os.environ["VSA_CHAIN_SMALLMAX"] = small
            os.environ["VSA_CHAIN_WAVEMAX"] = wave
            ch, ev, wall = measure(layout, res, opt)
            other = ch.chains()
            for k in ("problem", "number", "score", "start", "members"):
                assert np.array_equal(other[k], want[k]), (spec, k)
            s2 = ch.stats().asdict()
            ch.close()
            report(dict(case=name, kind=a.kind, records=len(rec),
                        bounds=spec, classes={k: s2[k] for k in (
                            "single", "small", "wave", "group")},
                        event_ms={k: both(v) for k, v in ev.items()},
                        wall_ms={k: both(v) for k, v in wall.items()}))
            del os.environ["VSA_CHAIN_SMALLMAX"]
            del os.environ["VSA_CHAIN_WAVEMAX"]
        res.close()


if __name__ == "__main__":
    main()
