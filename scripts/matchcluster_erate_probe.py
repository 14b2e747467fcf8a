#!/usr/bin/env python3
"""Match clustering by edit distance (vmatch -pp matchcluster erate E) at
list sizes of 10^4, 10^5 and 10^6 matches (and 2 000 first, for a pair rate
to predict the next size from): what vsa_matchcluster_add and
_finish cost on the device, stage by stage, next to what a caller has to do
without them -- vsa_result_fetch of the list plus the reference's two loops
on the host (vsa_eratecluster_host).

usage: matchcluster_erate_probe.py [--sizes N,N,...] [--erate E]
                                   [--families F]
                                   [--budget-s S] [--host-pairs P]
                                   [--out FILE]
The text is synthetic: FAMILIES families of four near-copies (3 % of the
symbols substituted) of a random stretch of 1100 symbols.  Both instances of
a match are copies of one family at one of a few offsets, so matches of one
family are within reach of each other and all others are not.
  mixed      lengths 30..100: the length test rejects most pairs
  onelength  every match has LENGTH symbols, one case per width of the lane
             group of the distance kernel (LENGTH 50, 120, 250, 500, 1000
             with E = 10: bounds 5, 12, 25, 50, 100): every pair passes the
             length test, the pairs stage is the distance kernel, and
             pairs / pairs stage time is its pair rate at that width
The work is quadratic.  A case is run if the time predicted from the pair
rate of the same kind of list at the size before stays below --budget-s
(default 60); otherwise the record says "extrapolated" and holds that
prediction, nothing else.  The host code runs on the first matches of the
list, as many as give about --host-pairs pairs (default 2e6, fewer in
proportion to the square of bounds above 10); its time for the whole list is
that time scaled by the number of pairs, and the record says so.  The
device's answer for those first matches is compared with the host's.  Prints
one JSON line per case (and appends it to FILE).  Needs no reference program.
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

BASE, COPIES, OFFSETS = 1100, 4, (0, 1, 2, 40)
WIDTHS = ((50, "16 lanes"), (120, "32 lanes"), (250, "64 lanes"),
          (500, "64 lanes x 2"), (1000, "64 lanes x 4"))


def make_text(families, seed=5):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 4, (families, 1, BASE), dtype=np.uint8)
    text = np.repeat(base, COPIES, axis=1)
    flip = rng.random(text.shape) < 0.03
    text = np.where(flip, (text + 1) % 4, text).astype(np.uint8)
    return text.reshape(-1)


def make_list(n, families, lengths, seed):
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, V.MATCH_DTYPE)
    rec["length"] = lengths(rng, n)
    fam = rng.integers(0, families, n)
    off = rng.choice(OFFSETS, n)
    for field in ("dbstart", "queryseq"):
        rec[field] = (fam * COPIES + rng.integers(0, COPIES, n)) * BASE + off
    return rec


def device_run(layout, index, E, res):
    mc = V.MatchCluster.erate(layout, index, E)
    V.device_synchronize()
    t0 = time.perf_counter()
    mc.add(res)
    t1 = time.perf_counter()
    mc.finish()
    t2 = time.perf_counter()
    return mc, dict(add=(t1 - t0) * 1e3, finish=(t2 - t1) * 1e3)


def host_prefix(n, pairs):
    return int(min(n, max(2, (2 * pairs) ** 0.5)))


def probe(kind, rec, layout, index, text, E, hostpairs, more):
    n = len(rec)
    d = dict(case=kind, erate=E, matches=n, pairs=n * (n - 1) // 2, **more)
    res = V.Result.from_host(rec)
    try:
        warm = V.Result.from_host(rec[:1000])   # loads the kernels
        device_run(layout, index, E, warm)[0].close()
        warm.close()
        mc, wall = device_run(layout, index, E, res)
    except V.VsaError as e:
        d["error"] = "%d: %s" % (e.code, e.message)
        return d
    st = mc.stats().asdict()
    ev = mc.times()
    d.update(stats=st, event_ms={k: round(v, 3) for k, v in ev.items()},
             wall_ms={k: round(v, 3) for k, v in wall.items()},
             device_wall_ms=round(sum(wall.values()), 3),
             pairs_per_second_pairs_stage=round(
                 d["pairs"] / (ev["pairs"] * 1e-3)) if ev["pairs"] > 0
             else None)
    mc.close()
    t0 = time.perf_counter()
    fetched = res.fetch()
    d["fetch_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    # the host on the first k matches, and the device on the same
    # (a scalar front costs about the square of its bound)
    bound = max(1, int(rec["length"].max()) * E // 100)
    k = host_prefix(n, hostpairs / max(1.0, (bound / 10.0) ** 2))
    part = V.MatchCluster.erate(layout, index, E)
    part.add(V.Result.from_host(fetched[:k]))
    part.finish()
    got = part.edges()
    # ONE call of the C entry, with room for the edges the device found
    t0 = time.perf_counter()
    want = V.matchcluster_erate_host(layout, E, text, fetched[:k], text=False,
                                     edges=len(got[1]) + 1)
    hostms = (time.perf_counter() - t0) * 1e3
    for a, key in zip(got, ("edgestart", "m0", "m1", "values")):
        assert np.array_equal(a, want[key]), key
    assert np.array_equal(part.members()[1], want["members"])
    part.close()
    scale = d["pairs"] / (k * (k - 1) // 2)
    d.update(host_matches=k, host_pairs=k * (k - 1) // 2,
             host_ms_measured=round(hostms, 3),
             host_ms_extrapolated_by_pairs=round(hostms * scale, 1),
             host_is_extrapolated=bool(k < n), equal_to_host_on_prefix=True,
             ratio_fetch_plus_host_over_device=round(
                 (d["fetch_ms"] + hostms * scale) / d["device_wall_ms"], 1))
    res.close()
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2e3,1e4,1e5,1e6")
    ap.add_argument("--erate", type=int, default=10)
    ap.add_argument("--families", type=int, default=2000)
    ap.add_argument("--budget-s", type=float, default=60.0)
    ap.add_argument("--host-pairs", type=float, default=2e6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if V.device_count() < 1:
        sys.exit("matchcluster_erate_probe.py needs a GPU")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def report(d):
        print(json.dumps(d), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(d) + "\n")

    text = make_text(a.families)
    index = V.Index.build(text, 4, 0, 0)
    layout = V.sink_params(kind=V.SINK_SELF, totallength=len(text),
                           markpos=[])
    sizes = [int(float(x)) for x in a.sizes.split(",")]
    kinds = [("mixed", lambda rng, n: rng.integers(30, 101, n), {})] + [
        ("onelength", (lambda L: lambda rng, n: np.full(n, L))(L),
         dict(length=L, group=group)) for L, group in WIDTHS]
    for kind, lengths, more in kinds:
        rate = None                  # seconds per pair at the size before
        for n in sizes:
            pairs = n * (n - 1) // 2
            if rate is not None and rate * pairs > a.budget_s:
                report(dict(case=kind, erate=a.erate, matches=n, pairs=pairs,
                            extrapolated=True, predicted_device_s=round(
                                rate * pairs, 1),
                            from_the_pair_rate_of_the_size_before=True,
                            **more))
                continue
            d = probe(kind, make_list(n, a.families, lengths, n), layout,
                      index, text, a.erate, a.host_pairs, more)
            report(d)
            if "error" in d:
                break
            rate = d["device_wall_ms"] * 1e-3 / pairs


if __name__ == "__main__":
    main()
