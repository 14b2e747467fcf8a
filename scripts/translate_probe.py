#!/usr/bin/env python3
"""DNA reads against a protein index in six frames (vmatch -dnavsprot) on the
GPU: what translation, search and conversion cost.

usage: translate_probe.py [NQ [M [N [L]]]] [--out FILE]
  NQ reads of M characters resident in HBM (default 1e7 x 150), a random
  20-letter index of N symbols from a fixed seed (default 1e8), -mum -l L
  (default 10).  One read in ten is the back-translation of a stretch of the
  index.
Prints one JSON line (and writes it to FILE): HIP-event times, after a
warm-up, of the translation kernels, of the -mum search on the six-frame batch
and of the conversion of its list; the rate of the translation -- it reads n
bytes and writes about 2 n -- as a share of what vsa_measure_stream_read
reports in the same run, and against vsa_translate_host on 16 threads.
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vstree_amd as V  # noqa: E402

AMINO = b"ACDEFGHIKLMNPQRSTVWY"
# one codon per amino acid (the standard code), for the planted reads
CODON = {"A": "GCT", "C": "TGT", "D": "GAT", "E": "GAA", "F": "TTT",
         "G": "GGT", "H": "CAT", "I": "ATT", "K": "AAA", "L": "CTG",
         "M": "ATG", "N": "AAT", "P": "CCT", "Q": "CAA", "R": "CGT",
         "S": "TCT", "T": "ACT", "V": "GTT", "W": "TGG", "Y": "TAT"}
HOST_THREADS = 16


def symbol_map():
    m = np.full(256, 253, np.uint8)
    for ch in b"BXZ*":
        m[ch] = V.WILDCARD
    for i, ch in enumerate(AMINO):
        m[ch] = m[ch + 32] = i
    return m


def make_reads(rng, tis, nq, m):
    bases = np.frombuffer(b"ACGT", np.uint8)
    reads = bases[V.synth_genome(nq * m, 4711)].reshape(nq, m)
    k = m // 3
    planted = np.arange(0, nq, 10)
    pos = rng.integers(0, len(tis) - k, len(planted))
    aa = tis[pos[:, None] + np.arange(k)[None, :]]
    table = np.array([list(CODON[chr(c)].encode()) for c in AMINO], np.uint8)
    reads[planted, :3 * k] = table[aa].reshape(len(planted), 3 * k)
    return np.ascontiguousarray(reads.reshape(-1))


def host_rate(chars, nq, m, symmap):
    """vsa_translate_host over HOST_THREADS shards at once -> seconds"""
    per = (nq + HOST_THREADS - 1) // HOST_THREADS

    def work(t):
        a, b = t * per, min(nq, (t + 1) * per)
        if a < b:
            start = np.arange(b - a, dtype=np.uint64) * np.uint64(m)
            V.translate_host(1, chars[a * m:b * m], start,
                             np.full(b - a, m, np.uint64), symmap)
    threads = [threading.Thread(target=work, args=(t,))
               for t in range(HOST_THREADS)]
    t0 = time.perf_counter()
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=float)
    ap.add_argument("--out")
    a = ap.parse_args()
    nq, m, n, L = [int(x) for x in
                   (a.sizes + [1e7, 150, 1e8, 10][len(a.sizes):])]
    rng = np.random.default_rng(20261019)
    symmap = symbol_map()
    tis = rng.integers(0, 20, n).astype(np.uint8)
    chars = make_reads(rng, tis, nq, m)
    index = V.Index.build(tis, 20, 0)
    d = V.device_malloc(nq * m)
    V.device_upload(d, chars)
    stream = V.measure_stream_read(1 << 30)

    def once():
        q = V.Queries.translate_device(1, d, nq, m, symmap)
        r = V.findquerymatches(index, q, L, mum=True)
        view, reverse = V.translated_convert(r, q)
        out = dict(translate_ms=q.translate_ms(),
                   search_ms=r.stats().total_device_ms,
                   convert_ms=view.stats().total_device_ms,
                   matches=r.count, reverse=int(reverse.sum()),
                   symbols=int(q.info().numofsymbols))
        for h in (view, r, q):
            h.close()
        return out

    once()                                        # warm-up
    runs = [once() for _ in range(2)]
    best = min(runs, key=lambda x: x["translate_ms"])
    nbytes = nq * m + best["symbols"]             # read n, write about 2 n
    gbps = nbytes / best["translate_ms"] / 1e6
    hq = min(nq, 1000000)                         # the host: a tenth is enough
    host_s = host_rate(chars, hq, m, symmap)
    res = dict(probe="translate", nq=nq, m=m, n=n, L=L,
               prefixlength=int(index.info().prefixlength), **best,
               translate_ms_runs=[x["translate_ms"] for x in runs],
               search_ms_runs=[x["search_ms"] for x in runs],
               convert_ms_runs=[x["convert_ms"] for x in runs],
               translate_bytes=nbytes, translate_gbps=gbps,
               stream_read_gbps=stream,
               share_of_stream_read=gbps / stream,
               host_threads=HOST_THREADS, host_reads=hq,
               host_mchars_per_s=hq * m / host_s / 1e6,
               gpu_mchars_per_s=nq * m / best["translate_ms"] / 1e3,
               gpu_over_host=(nq * m / best["translate_ms"] / 1e3) /
                             (hq * m / host_s / 1e6))
    V.device_free(d)
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
