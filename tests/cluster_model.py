"""A pure-Python model of vmatch -dbcluster percsmall perclarge
(Vmatch/vmcluster.c:289-415, kurtz/cluster.c:436-683): which records of a
match list are edges between sequences, linkcluster, the numbering and member
order of showClusterSet, the printed lines and the order of the edges in the
per-cluster match files.  Two replays: every edge in order (full), and only
the edges of the minimum spanning forest with the edge number as weight
(forest) -- an edge changes the state of linkcluster only if its ends are in
different clusters at that moment, and Kruskal takes exactly those.  Written
from the reference's text, independently of the library's C code."""
import numpy as np

SINGLET = 2 ** 64 - 1
EDGE, BAD, SAME, MIRROR, REJECTED = range(5)


class Layout:
    def __init__(self, totallength, markpos):
        self.totallength = int(totallength)
        self.markpos = np.asarray(markpos, np.int64)
        self.numofsequences = len(self.markpos) + 1
        self.start = np.concatenate(([0], self.markpos + 1))
        self.end = np.concatenate((self.markpos, [self.totallength]))
        self.seqlen = self.end - self.start


def seqof(lay, pos, length):
    """the sequence [pos, pos + length) lies in, or None"""
    if length == 0 or pos + length > lay.totallength:
        return None
    s = int(np.searchsorted(lay.markpos, pos, "left"))
    if pos < lay.start[s] or pos + length > lay.end[s]:
        return None
    return s


def classify(lay, rec, pal, percsmall, perclarge):
    """one record (length, dbstart, queryseq, querystart) -> (class, seq1,
    seq2)"""
    length, dbstart, queryseq, querystart = (int(x) for x in rec)
    s1 = seqof(lay, dbstart, length)
    if s1 is None:
        return BAD, None, None
    if pal:
        s2 = queryseq
        if s2 >= lay.numofsequences or \
                querystart + length > int(lay.seqlen[s2]):
            return BAD, None, None
    else:
        s2 = seqof(lay, queryseq, length)
        if s2 is None:
            return BAD, None, None
    if s1 == s2:
        return SAME, s1, s2
    if pal and s1 > s2:
        return MIRROR, s1, s2
    small, large = sorted((int(lay.seqlen[s1]), int(lay.seqlen[s2])))
    if length >= small * percsmall // 100 and \
            length >= large * perclarge // 100:
        return EDGE, s1, s2
    return REJECTED, s1, s2


def edges_of(lay, rec, flags, percsmall, perclarge):
    """-> (edges [(seq1, seq2)], the record of each edge, counts per class);
    ValueError for a record that does not fit"""
    edges, src, counts = [], [], [0] * 5
    for i, r in enumerate(rec):
        c, s1, s2 = classify(lay, (r["length"], r["dbstart"], r["queryseq"],
                                   r["querystart"]),
                             bool(flags[i]) if flags is not None else False,
                             percsmall, perclarge)
        if c == BAD:
            raise ValueError("record %d does not fit the layout" % i)
        counts[c] += 1
        if c == EDGE:
            edges.append((s1, s2))
            src.append(i)
    return edges, src, counts


class ClusterSet:
    """kurtz/cluster.c: celems (clusternumber, nextelem), cinfo (csize,
    firstelem, lastelem)"""

    def __init__(self, numofelems):
        self.cnum = [None] * numofelems
        self.next = [None] * numofelems
        self.csize, self.first, self.last = [], [], []

    def link(self, e1, e2):
        """linkcluster -> True if the edge joined two different clusters"""
        c1, c2 = self.cnum[e1], self.cnum[e2]
        if c1 is None and c2 is None:
            c = len(self.csize)
            self.cnum[e1] = self.cnum[e2] = c
            self.next[e1], self.next[e2] = e2, None
            self.csize.append(2)
            self.first.append(e1)
            self.last.append(e2)
            return True
        if c1 is None or c2 is None:
            c, e = (c2, e1) if c1 is None else (c1, e2)
            self.cnum[e], self.next[e] = c, None
            self.next[self.last[c]] = e
            self.last[c] = e
            self.csize[c] += 1
            return True
        if c1 == c2:
            return False
        target, source = (c1, c2) if self.csize[c1] > self.csize[c2] \
            else (c2, c1)
        i = self.first[source]
        while i is not None:
            self.cnum[i] = target
            i = self.next[i]
        self.next[self.last[target]] = self.first[source]
        self.first[source] = None
        self.last[target] = self.last[source]
        self.csize[target] += self.csize[source]
        self.csize[source] = 0
        return True

    def clusters(self):
        """showClusterSet: the member lists in output numbering"""
        out = []
        for c, size in enumerate(self.csize):
            if size > 0:
                mem, i = [], self.first[c]
                while i is not None:
                    mem.append(i)
                    i = self.next[i]
                assert len(mem) == size
                out.append(mem)
        return out


def full_replay(numofsequences, edges):
    """-> (clusters, the numbers of the edges that changed the state)"""
    cs = ClusterSet(numofsequences)
    changed = [i for i, (a, b) in enumerate(edges) if cs.link(a, b)]
    return cs.clusters(), changed


def forest_of(numofsequences, edges):
    """Kruskal with weight = edge number -> the numbers of the forest edges"""
    parent = list(range(numofsequences))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    out = []
    for i, (a, b) in enumerate(edges):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
            out.append(i)
    return out


def forest_replay(numofsequences, edges):
    forest = forest_of(numofsequences, edges)
    cs = ClusterSet(numofsequences)
    for i in forest:
        assert cs.link(*edges[i])
    return cs.clusters(), forest


def labels_of(numofsequences, clusters):
    lab = np.full(numofsequences, SINGLET, np.uint64)
    for c, mem in enumerate(clusters):
        lab[mem] = c
    return lab


def group_edges(numofsequences, clusters, edges):
    """addClusterEdge: -> (edgestart, edge numbers grouped by cluster, each
    cluster's in descending order)"""
    lab = labels_of(numofsequences, clusters)
    per = [[] for _ in clusters]
    for i, (a, b) in enumerate(edges):
        assert lab[a] == lab[b] != SINGLET
        per[int(lab[a])].append(i)
    start, order = [0], []
    for p in per:
        order += p[::-1]
        start.append(len(order))
    return np.array(start, np.uint64), np.array(order, np.uint64)


def format_text(numofsequences, clusters):
    """clusterSizedistribution and the cluster lines of processvmcluster"""
    k = len(clusters)
    csum = sum(len(m) for m in clusters)
    out = ["# %d cluster%s" % (k, "" if k == 1 else "s"),
           "# %d elements out of %d (%.2f%%) are in clusters"
           % (csum, numofsequences, 100.0 * csum / numofsequences),
           "# %d elements out of %d (%.2f%%) are singlets"
           % (numofsequences - csum, numofsequences,
              100.0 * (numofsequences - csum) / numofsequences)]
    dist = {}
    for m in clusters:
        dist[len(m)] = dist.get(len(m), 0) + 1
    for size in sorted(dist):
        out.append("# %d cluster%s of size %d"
                   % (dist[size], "s" if dist[size] > 1 else "", size))
    for c, m in enumerate(clusters):
        out.append("%d: " % c + "".join(" %d" % e for e in m))
    return ("\n".join(out) + "\n").encode()


def cluster(lay, rec, flags, percsmall, perclarge, replay=full_replay):
    """-> dict like vstree_amd.cluster_host returns, stats as a dict"""
    edges, src, counts = edges_of(lay, rec, flags, percsmall, perclarge)
    clusters, forest = replay(lay.numofsequences, edges)
    estart, eorder = group_edges(lay.numofsequences, clusters, edges)
    inclusters = sum(len(m) for m in clusters)
    start = np.cumsum([0] + [len(m) for m in clusters]).astype(np.uint64)
    return dict(
        stats=dict(seen=len(rec), samesequence=counts[SAME],
                   mirrordropped=counts[MIRROR], rejected=counts[REJECTED],
                   edges=len(edges), forestedges=len(forest), rounds=0,
                   clusters=len(clusters), inclusters=inclusters,
                   singlets=lay.numofsequences - inclusters),
        clusters=clusters, clusterstart=start,
        members=np.array([e for m in clusters for e in m], np.uint64),
        labels=labels_of(lay.numofsequences, clusters), edgestart=estart,
        edgerecord=np.array([src[int(i)] for i in eorder], np.uint64),
        text=format_text(lay.numofsequences, clusters))
