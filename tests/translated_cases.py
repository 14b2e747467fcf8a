"""Shared by tests/test_translated.py and tests/test_gpu_translated.py: the
fixtures of the six-frame translation (tests/golden/translated_*,
scripts/make_golden_translated.py), DNA batches as the translation takes them
and a numpy model of the coverage of their matches."""
import gzip
import json
import os

import numpy as np

import helpers as H

with open(os.path.join(H.GOLDEN, "translated_codons.json")) as f:
    CODONS = json.load(f)
with gzip.open(os.path.join(H.GOLDEN, "translated_runs.json.gz")) as f:
    RECORDED = json.load(f)
RUNS, L, NOMATCH = RECORDED["runs"], RECORDED["L"], RECORDED["nomatch"]
TABLES = sorted(int(t) for t in CODONS["plain"])
AMINO = CODONS["amino"]

# run -> (translation table, keyword arguments of the query engine)
MATCH_RUNS = {"mem": (1, {}), "mum": (1, dict(mum=True)),
              "mumcand": (1, dict(mum=True, cand=True)),
              "mem_absolute": (1, {}), "mem_table4": (4, {})}
SHOW_ABSOLUTE = 1


def lines_of(key):
    return "".join(l + "\n" for l in RUNS[key]["lines"]).encode()


def codon_list(letters):
    return [a + b + c for a in letters for b in letters for c in letters]


def amino_map():
    """symbol map of an alphabet whose codes are the places in AMINO; every
    other letter and '*' are its wildcard (what mkvtree -protein does with
    them: the recorded runs print no line for such a codon)"""
    m = np.full(256, 253, np.uint8)
    for ch in b"ABCDEFGHIKLMNPQRSTVWXYZ":
        m[ch] = m[ch + 32] = H.WILDCARD
    m[ord("*")] = H.WILDCARD
    for i, ch in enumerate(AMINO.encode()):
        m[ch] = m[ch + 32] = i
    return m


def letters_of(symbols):
    """codes of amino_map() -> str, '*' for the wildcard"""
    table = np.full(256, ord("?"), np.uint8)
    table[:len(AMINO)] = np.frombuffer(AMINO.encode(), np.uint8)
    table[H.WILDCARD] = ord("*")
    return table[np.asarray(symbols, np.uint8)].tobytes().decode()


class Dna:
    """DNA sequences as the translation takes them: characters, one 0xFF
    between two sequences, and the Multiseq the reference lays out"""

    def __init__(self, seqs):
        self.seqs = [s if isinstance(s, bytes) else s.encode() for s in seqs]
        self.length = np.array([len(s) for s in self.seqs], np.uint64)
        self.start = (np.concatenate(([0], np.cumsum(self.length + 1)[:-1]))
                      .astype(np.uint64) if self.seqs
                      else np.zeros(0, np.uint64))
        self.chars = np.frombuffer(b"\xff".join(self.seqs), np.uint8)
        self.totallength = int(self.length.sum()) + max(len(self.seqs) - 1, 0)

    @property
    def nq(self):
        return len(self.seqs)

    @staticmethod
    def fasta(name):
        return Dna([s for _, s in H.read_fasta(H._golden_fasta(name))])


def expected_frames(length):
    """(start, length) of the six frames of every sequence, from the closed
    forms of the issue: frame f and reverse frame r have (len - f) / 3
    symbols, 0 where len < f; a separator behind every frame but the last"""
    ps, pl, pos = [], [], 0
    for n in (int(x) for x in length):
        for f in (0, 1, 2, 0, 1, 2):
            k = (n - f) // 3 if n >= f else 0
            ps.append(pos)
            pl.append(k)
            pos += k + 1
    return np.array(ps, np.uint64), np.array(pl, np.uint64), max(pos - 1, 0)


def host_batch(V, dna, transnum, symmap):
    """the six-frame batch of the host translation as oracle queries"""
    sym, ps, pl = V.translate_host(transnum, dna.chars, dna.start, dna.length,
                                   symmap)
    return H.Queries(sym, ps, pl)


def sink(V, idx, dna, showmode=0, leastlength=L, complete=False):
    return V.Sink(V.SINK_TRANSLATED_COMPLETE if complete
                  else V.SINK_TRANSLATED, idx.n, idx.ssp,
                  numofchars=idx.numofchars, querystart=dna.start,
                  querylength=dna.length, querytotallength=dna.totallength,
                  leastlength=leastlength, showmode=showmode)


def layout(V, idx, dna):
    return V.sink_params(V.SINK_TRANSLATED, idx.n, idx.ssp,
                         numofchars=idx.numofchars, querystart=dna.start,
                         querylength=dna.length,
                         querytotallength=dna.totallength, leastlength=L)


def unmarked_runs(nbits, separators, starts, lengths, minlength, last=None):
    """the numpy model of a coverage: bits set for [starts[i], +lengths[i])
    and for the separators -> INTERVAL records of the clear runs of at least
    minlength positions in [0, last)"""
    marked = np.zeros(nbits + 1, bool)
    sep = np.asarray(separators, np.int64)
    marked[sep] = True
    for s, n in zip(starts, lengths):
        marked[int(s):int(s) + int(n)] = True
    last = nbits if last is None else last
    marked[last:] = True
    d = np.diff(np.concatenate(([0], (~marked).astype(np.int8), [0])))
    s, e = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    keep = e - s >= minlength
    s, e = s[keep], e[keep]
    seq = np.searchsorted(sep, s, side="left")
    seqstart = np.concatenate(([0], sep + 1))[seq]
    out = np.zeros(len(s), H.MATCH_DTYPE)
    out["length"], out["dbstart"] = e - s, s
    out["queryseq"], out["querystart"] = seq, s - seqstart
    return out


def query_runs(dna, view):
    """-qnomatch: the clear runs of the DNA Multiseq under the query view"""
    sep = (dna.start[1:] - np.uint64(1)).astype(np.int64)
    q = view["queryseq"].astype(np.int64)
    return unmarked_runs(dna.totallength, sep,
                         dna.start[q] + view["querystart"], view["length"],
                         NOMATCH)


def database_runs(idx, matches):
    """-dbnomatch: the clear runs of the index under the unconverted list
    (with -q the reference scans the whole table, Vmatch/initpost.c:181-190)"""
    return unmarked_runs(idx.n, idx.ssp.astype(np.int64), matches["dbstart"],
                         matches["length"], NOMATCH)
