"""A pure-Python model of vmatch -pp matchcluster gapsize G | overlap P
(Vmatch/clpos.c:14-201, Vmatch/matchclust.c:10-128): the two references of
every match sorted by their start, the two nested loops that link them, the
edges through linkcluster, and the printed lines.  linkcluster, the numbering
of showClusterSet, the forest and the order of addClusterEdge are those of
cluster_model.py with the matches as elements.  Written from the reference's
text, independently of the library's C code: the loops are the reference's
loops, not the windows the kernels use."""
import struct

import numpy as np

import cluster_model as CM

GAP, OVERLAP = 0, 1
MASK = 2 ** 64 - 1


def view(kind, rec, flags=None, querystart=None, querylength=None,
         dblenplus1=0):
    """what processfinal stores of the records of a list -> (length1,
    position1, position2) as lists of int.  kind 2: a self list (position2 =
    the second start, minus dblenplus1 on an index with queries); else a list
    against queries: position2 = the start of the query sequence plus the
    offset, counted from the other end for a palindromic record; length1 =
    the length on the database side."""
    l1 = [int(x) for x in rec["length"]]
    p1 = [int(x) for x in rec["dbstart"]]
    if kind == 2:
        p2 = [int(x) - dblenplus1 for x in rec["queryseq"]]
        return l1, p1, p2
    p2 = []
    for i, r in enumerate(rec):
        q = int(r["queryseq"])
        seqlen, rel = int(querylength[q]), int(r["querystart"])
        length2 = int(r["length"]) if kind == 1 else seqlen
        if kind != 1:
            rel = 0
        if flags is not None and flags[i]:
            rel = seqlen - (rel + length2)
        p2.append(int(querystart[q]) + rel)
    return l1, p1, p2


def references(p1, p2):
    """mirrorandsortmatches: (start, match) sorted by start alone, equal
    starts in the order of their index (a merging qsort is stable)"""
    ref = []
    for m in range(len(p1)):
        ref.append((p1[m], m))
        ref.append((p2[m], m))
    return sorted(ref, key=lambda r: r[0])


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def edges_of(l1, p1, p2, mode, value):
    """-> (edges [(m_i, m_j, gap or overlap)], counts dict)"""
    ref = references(p1, p2)
    edges, cand, same, below = [], 0, 0, 0
    for i in range(len(ref) - 1):
        si, mi = ref[i]
        end = si + l1[mi]
        for j in range(i + 1, len(ref)):
            sj, mj = ref[j]
            if mode == GAP:
                gap = (sj - end) & MASK
                if gap > value:
                    break
                cand += 1
                if mi != mj:
                    edges.append((mi, mj, gap))
                else:
                    same += 1
            else:
                if end < sj:
                    break
                cand += 1
                if mi == mj:
                    same += 1
                    continue
                longer = l1[mi] if l1[mi] >= l1[mj] else l1[mj]
                overlap = (float(end - sj) * 100.0) / float(longer)
                if overlap >= float(value):
                    edges.append((mi, mj, overlap))
                else:
                    below += 1
    return edges, dict(candidates=cand, samematch=same, below=below)


def format_text(n, clusters):
    out = ["# cluster %d matches" % n]
    out += ["# create cluster %d of size %d" % (c, len(m))
            for c, m in enumerate(clusters)]
    return ("\n".join(out) + "\n").encode()


def printed_ids(flags):
    """the number the reference prints for match m: its idnumber, which
    starts again at 0 with the P pass of a -d -p run, although the clustering
    itself goes by the place in the buffer"""
    ids, first = [], 0
    for m, f in enumerate(flags):
        if m > 0 and f != flags[m - 1]:
            first = m
        ids.append(m - first)
    return ids


def format_cluster(mode, members, lines, edges, ids=None):
    """the bytes of PREFIX.size.c.match behind its first line; lines[t]: the
    match line of members[t] without its newline; edges in file order; ids:
    printed_ids of the list, where it has more than one pass"""
    out = []
    name = (lambda m: m) if ids is None else (lambda m: ids[m])
    for m, line in zip(members, lines):
        out.append("# id %d" % name(m))
        out.append(line)
    for a, b, v in edges:
        out.append("# linked %d and %d with " % (name(a), name(b)) +
                   ("gapsize %d" % v if mode == GAP
                    else "overlap percentage %.2f" % v))
    return ("\n".join(out) + "\n").encode()


def cluster(l1, p1, p2, mode, value, replay=CM.full_replay):
    """-> dict like vstree_amd.matchcluster_host returns, stats as a dict,
    values as 64-bit patterns; edges: per cluster, in file order"""
    n = len(l1)
    edges, counts = edges_of(l1, p1, p2, mode, value)
    pairs = [(a, b) for a, b, _ in edges]
    clusters, forest = replay(n, pairs)
    estart, eorder = CM.group_edges(n, clusters, pairs)
    grouped = [edges[int(i)] for i in eorder]
    inclusters = sum(len(m) for m in clusters)
    stats = dict(matches=n, edges=len(edges), forestedges=len(forest),
                 rounds=0, clusters=len(clusters), inclusters=inclusters)
    stats.update(counts)
    return dict(
        stats=stats, clusters=clusters,
        clusterstart=np.cumsum([0] + [len(m) for m in clusters]).astype(
            np.uint64),
        members=np.array([e for m in clusters for e in m], np.uint64),
        labels=CM.labels_of(n, clusters), edgestart=estart,
        m0=np.array([e[0] for e in grouped], np.uint32),
        m1=np.array([e[1] for e in grouped], np.uint32),
        values=np.array([e[2] if mode == GAP else bits(e[2])
                         for e in grouped], np.uint64),
        edges=[grouped[int(estart[c]):int(estart[c + 1])]
               for c in range(len(clusters))],
        text=format_text(n, clusters))
