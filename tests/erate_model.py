"""A pure-Python model of vmatch -pp matchcluster erate E
(Vmatch/cluedist.c:42-198, kurtz/frontSEP.c:341-446, kurtz/front.gen:48-213,
Vmatch/matchclust.c:10-128): every pair i < j of a self list, the bound from
the shorter match, the cascade over the four instance pairs, the edges through
linkcluster and the printed lines.  linkcluster, the numbering, the forest and
the order of a cluster's edges are those of cluster_model.py with the matches
as elements.  Written from the reference's text, independently of the
library's C code.

Two statements of the answer of one instance pair:

  dp_answer     a plain quadratic DP of the unit edit distance in which a
                special symbol (>= 254) equals nothing, not even itself.
  front_answer  the reference's greedy front, round by round.  It differs
                from the DP in one thing, which what the reference prints
                depends on: in a round d >= 1 a diagonal on which both
                substrings are the same text (pu + t == pv + t + k) is not
                slid along, its row becomes ulen - 1 (front.gen:120-123).
                That can only happen where the two instances start at most
                maxdist apart; for every other instance pair both statements
                must agree, which the tests check.

batch_answers is front_answer over arrays of instance pairs at once (numpy):
the recorded runs look at up to 10 million pairs."""
import numpy as np

import cluster_model as CM
import matchcluster_model as MM

SPECIAL = 254
NEG = -(1 << 40)


def maxdist(minlen, errorrate):
    return int(float(minlen) * float(errorrate) / 100.0)


def symequal(a, b):
    return a == b and a < SPECIAL


def dp_answer(text, pu, ulen, pv, vlen, md):
    """verifysmalldistance with a textbook distance"""
    if abs(ulen - vlen) > md:
        return -1
    if ulen == vlen and pu == pv:
        return 0
    u, v = text[pu:pu + ulen], text[pv:pv + vlen]
    row = list(range(vlen + 1))
    for a in range(1, ulen + 1):
        new = [a] + [0] * vlen
        for b in range(1, vlen + 1):
            new[b] = min(row[b] + 1, new[b - 1] + 1, row[b - 1] +
                         (0 if symequal(int(u[a - 1]), int(v[b - 1])) else 1))
        row = new
    return row[vlen] if row[vlen] <= md else -1


def may_differ(pu, pv, md):
    """an instance pair on which the front may leave the textbook"""
    return abs(pu - pv) <= md


def slide(text, pu, ulen, pv, vlen, t, k):
    while t < ulen and t + k < vlen and \
            symequal(int(text[pu + t]), int(text[pv + t + k])):
        t += 1
    return t


def front_answer(text, pu, ulen, pv, vlen, md):
    """verifysmalldistance and unitedistfrontSEPgeneric with a bound"""
    if abs(ulen - vlen) > md:
        return -1
    if ulen == vlen and pu == pv:
        return 0
    goal = vlen - ulen
    prev = {0: slide(text, pu, ulen, pv, vlen, 0, 0)}
    if goal == 0 and prev[0] == ulen:
        return 0
    for d in range(1, md + 1):
        cur = {}
        for k in range(-d, d + 1):
            t = max(prev.get(k, NEG) + 1, prev.get(k - 1, NEG),
                    prev.get(k + 1, NEG) + 1)
            if t < 0 or t + k < 0:
                cur[k] = NEG
                continue
            if ulen != 0 and vlen != 0 and pu + t == pv + t + k:
                t = ulen - 1
            else:
                t = slide(text, pu, ulen, pv, vlen, t, k)
            cur[k] = NEG if t > ulen or t + k > vlen else t
        if cur.get(goal, NEG) == ulen:
            return d
        prev = cur
    return -1


def _slide_many(text, pu, ulen, pv, vlen, t, k):
    t = t.copy()
    idx = np.arange(len(t))
    while len(idx):
        a = t[idx]
        idx = idx[(a < ulen[idx]) & (a + k[idx] < vlen[idx])]
        ca = text[pu[idx] + t[idx]]
        cb = text[pv[idx] + t[idx] + k[idx]]
        idx = idx[(ca == cb) & (ca < SPECIAL)]
        t[idx] += 1
    return t


def batch_answers(text, pu, ulen, pv, vlen, md):
    """front_answer for arrays of instance pairs (int64)"""
    P = len(pu)
    res = np.full(P, -1, np.int64)
    res[(ulen == vlen) & (pu == pv)] = 0
    live = np.flatnonzero((res < 0) & (np.abs(ulen - vlen) <= md))
    if len(live) == 0:
        return res
    pu, ulen, pv, vlen, md = (x[live] for x in (pu, ulen, pv, vlen, md))
    top = int(md.max())
    ks = np.arange(-top, top + 1, dtype=np.int64)
    front = np.full((len(live), 2 * top + 3), NEG, np.int64)
    zero = np.zeros(len(live), np.int64)
    front[:, top + 1] = _slide_many(text, pu, ulen, pv, vlen, zero, zero)
    out = np.full(len(live), -1, np.int64)
    out[(ulen == vlen) & (front[:, top + 1] == ulen)] = 0
    for d in range(1, top + 1):
        act = np.flatnonzero((out < 0) & (md >= d))
        if len(act) == 0:
            break
        F = front[act]
        t = np.maximum(np.maximum(F[:, 1:-1] + 1, F[:, :-2]), F[:, 2:] + 1)
        A = len(act)
        k2 = np.broadcast_to(ks, t.shape)
        b = [np.broadcast_to(x[act][:, None], t.shape)
             for x in (pu, ulen, pv, vlen)]
        valid = (t >= 0) & (t + k2 >= 0)
        same = valid & (b[1] != 0) & (b[3] != 0) & (b[0] == b[2] + k2)
        go = valid & ~same
        slid = _slide_many(text, b[0][go], b[1][go], b[2][go], b[3][go],
                           t[go], k2[go])
        t = np.where(same, b[1] - 1, t)
        t[go] = slid
        stored = np.where(valid & (t <= b[1]) & (t + k2 <= b[3]), t, NEG)
        front[act, 1:-1] = stored
        goal = (vlen - ulen)[act]
        hit = stored[np.arange(A), goal + top] == ulen[act]
        out[act[hit]] = d
    res[live] = out
    return res


def _pairs(l1, p1, p2, errorrate, i0, i1):
    """all pairs of the rows i0 .. i1 - 1 -> (i, j, bound) as arrays"""
    n = len(l1)
    ii = np.repeat(np.arange(i0, i1), n - 1 - np.arange(i0, i1))
    jj = np.concatenate([np.arange(i + 1, n) for i in range(i0, i1)]
                        or [np.zeros(0, np.int64)])
    minlen = np.minimum(l1[ii], l1[jj])
    md = (minlen.astype(np.float64) * float(errorrate) / 100.0) \
        .astype(np.int64)
    return ii, jj, minlen, md


def edges_of(text, l1, p1, p2, errorrate, answer=None, rows=400000):
    """-> (edges [(i, j, minlen, distance)] in the order found, counts).
    answer: front_answer or dp_answer pair by pair, or None: batch_answers"""
    n = len(l1)
    edges = []
    if answer is not None:
        for i in range(n):
            for j in range(i + 1, n):
                minlen = min(l1[i], l1[j])
                md = maxdist(minlen, errorrate)
                for pu, pv in ((p1[i], p1[j]), (p1[i], p2[j]),
                               (p2[i], p1[j]), (p2[i], p2[j])):
                    e = answer(text, pu, l1[i], pv, l1[j], md)
                    if e >= 0:
                        edges.append((i, j, minlen, e))
                        break
    else:
        text = np.asarray(text, np.uint8)
        L = np.asarray(l1, np.int64)
        pos = (np.asarray(p1, np.int64), np.asarray(p2, np.int64))
        i0 = 0
        while i0 < n - 1:
            i1, total = i0, 0
            while i1 < n - 1 and (i1 == i0 or total + n - 1 - i1 <= rows):
                total += n - 1 - i1
                i1 += 1
            ii, jj, minlen, md = _pairs(L, pos[0], pos[1], errorrate, i0, i1)
            ans = np.full(len(ii), -1, np.int64)
            for c in range(4):
                w = np.flatnonzero(ans < 0)
                ans[w] = batch_answers(text, pos[c >> 1][ii[w]], L[ii[w]],
                                       pos[c & 1][jj[w]], L[jj[w]], md[w])
            w = np.flatnonzero(ans >= 0)
            edges += list(zip(ii[w].tolist(), jj[w].tolist(),
                              minlen[w].tolist(), ans[w].tolist()))
            i0 = i1
    cand = n * (n - 1) // 2
    return edges, dict(candidates=cand, samematch=0, below=cand - len(edges))


def value(minlen, edist):
    return minlen << 32 | edist


def edge_line(a, b, v):
    minlen, edist = v >> 32, v & 0xFFFFFFFF
    return "# linked %d and %d with edit distance %d (error rate %.2f%%)" % (
        a, b, edist, 100.00 * float(edist) / minlen)


def format_cluster(members, lines, edges):
    """the bytes of PREFIX.size.c.match behind its first line; edges:
    (a, b, value) in file order"""
    out = []
    for m, line in zip(members, lines):
        out.append("# id %d" % m)
        out.append(line)
    out += [edge_line(a, b, v) for a, b, v in edges]
    return ("\n".join(out) + "\n").encode()


def cluster(text, l1, p1, p2, errorrate, replay=CM.full_replay, answer=None):
    """-> dict like vstree_amd.matchcluster_erate_host returns, stats as a
    dict; edges: per cluster (a, b, value), in file order"""
    n = len(l1)
    found, counts = edges_of(text, l1, p1, p2, errorrate, answer)
    edges = [(a, b, value(m, e)) for a, b, m, e in found]
    pairs = [(a, b) for a, b, _ in edges]
    clusters, forest = replay(n, pairs)
    estart, eorder = CM.group_edges(n, clusters, pairs)
    grouped = [edges[int(i)] for i in eorder]
    stats = dict(matches=n, edges=len(edges), forestedges=len(forest),
                 rounds=0, clusters=len(clusters),
                 inclusters=sum(len(m) for m in clusters))
    stats.update(counts)
    return dict(
        stats=stats, clusters=clusters,
        clusterstart=np.cumsum([0] + [len(m) for m in clusters]).astype(
            np.uint64),
        members=np.array([e for m in clusters for e in m], np.uint64),
        labels=CM.labels_of(n, clusters), edgestart=estart,
        m0=np.array([e[0] for e in grouped], np.uint32),
        m1=np.array([e[1] for e in grouped], np.uint32),
        values=np.array([e[2] for e in grouped], np.uint64),
        edges=[grouped[int(estart[c]):int(estart[c + 1])]
               for c in range(len(clusters))],
        text=MM.format_text(n, clusters))
