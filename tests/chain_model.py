"""A pure-Python model of vmatch -pp chain (Vmatch/chainvm.c,
kurtz-basic/chain2dim.c, kurtz/matsort.c): how the records of a list are
grouped into chaining problems and ordered inside one, what a fragment is,
how every fragment finds its predecessor and its score, which chains are
retrieved and what is printed.  The scores exist twice: as the literal sweep
over start and end points with a sorted list in the place of the red-black
tree (scores_sweep), and as the rule without any order of events that the
kernels use (scores_rule).  Integers are Python's; the two expressions on
doubles are written as the reference writes them."""
import bisect

GLOBAL, GLOBAL_GC, GLOBAL_OV, LOCAL_MAX, LOCAL_THRESHOLD, LOCAL_BEST, \
    LOCAL_PERCENT = range(7)
LOCAL_KINDS = (LOCAL_MAX, LOCAL_THRESHOLD, LOCAL_BEST, LOCAL_PERCENT)
UNDEF = -1
MASK64 = (1 << 64) - 1


# ---- grouping (kurtz/matsort.c:316-367, include/qsort.gen) ------------------

def quicksort(perm, lo, hi, key):
    """the quicksort of qsort.gen on perm[lo .. hi] by key[perm[.]]: median
    of three, the pivot parked at hi - 1, runs of at most 10 by insertion
    sort.  Not stable: equal keys of a wider run are shuffled."""
    stack = []
    left, right = lo, hi

    def gt(a, b):
        return key[a] > key[b]

    while True:
        width = right - left + 1
        if width > 10:
            mid = left + ((right - left) >> 1)
            if gt(perm[left], perm[mid]):
                perm[left], perm[mid] = perm[mid], perm[left]
            if gt(perm[mid], perm[right]):
                perm[mid], perm[right] = perm[right], perm[mid]
            if gt(perm[left], perm[mid]):
                perm[left], perm[mid] = perm[mid], perm[left]
            perm[mid], perm[right - 1] = perm[right - 1], perm[mid]
            pivot = key[perm[right - 1]]
            i, j = left, right - 1
            while True:
                i += 1
                while key[perm[i]] < pivot:
                    i += 1
                j -= 1
                while pivot < key[perm[j]]:
                    j -= 1
                if i >= j:
                    break
                perm[i], perm[j] = perm[j], perm[i]
            perm[i], perm[right - 1] = perm[right - 1], perm[i]
            if i - left > right - i:
                stack.append((left, i - 1))
                left = i + 1
            else:
                stack.append((i + 1, right))
                right = i - 1
            continue
        if width == 2:
            if gt(perm[left], perm[right]):
                perm[left], perm[right] = perm[right], perm[left]
        elif width > 2:
            for i in range(left + 1, right + 1):
                item = perm[i]
                k = i
                while True:
                    if key[item] >= key[perm[k - 1]]:
                        break
                    perm[k] = perm[k - 1]
                    k -= 1
                    if k == left:
                        break
                perm[k] = item
        if not stack:
            return
        left, right = stack.pop()


def group_by_seqnum(seq1, seq2, stable=False):
    """groupmatchesbyseqnum: a stable counting sort by seq1, the quicksort by
    seq2 inside every run -> the permutation.  stable=True: what a stable
    sort by (seq1, seq2) would leave instead"""
    n = len(seq1)
    if stable:
        return sorted(range(n), key=lambda m: (seq1[m], seq2[m]))
    perm = sorted(range(n), key=lambda m: seq1[m])
    start = 0
    for i in range(1, n + 1):
        if i == n or seq1[perm[i - 1]] != seq1[perm[i]]:
            if start < i - 1:
                quicksort(perm, start, i - 1, seq2)
            start = i
    return perm


def problems(seq1, seq2, pos2, withinborders, stable=False):
    """-> the chaining problems, each the list of its record numbers in the
    order of its fragments (chainvm.c:180-222,406-500)"""
    n = len(seq1)
    if n == 0:
        return []
    onepair = all(seq1[m] == seq1[0] and seq2[m] == seq2[0] for m in range(n))
    if not withinborders or onepair:
        groups = [list(range(n))]
    else:
        perm = group_by_seqnum(seq1, seq2, stable)
        groups = [[perm[0]]]
        for a, b in zip(perm, perm[1:]):
            if (seq1[a], seq2[a]) != (seq1[b], seq2[b]):
                groups.append([])
            groups[-1].append(b)
    # glibc's qsort merges: stable
    return [sorted(g, key=lambda m: pos2[m]) for g in groups]


def tie_runs(seq1, seq2, pos2, grouped):
    """runs of two or more records with the same (seq1, seq2, position2), or
    the same position2 where the list is one problem"""
    keys = sorted((seq1[m], seq2[m], pos2[m]) if grouped else pos2[m]
                  for m in range(len(pos2)))
    return sum(1 for i in range(1, len(keys)) if keys[i] == keys[i - 1] and
               (i == 1 or keys[i - 2] != keys[i]))


def replayed(seq1, seq2, pos2, grouped):
    """records in seq1 runs of more than 10 records that hold a tie run: the
    only ones the quicksort may leave in another than the stable order"""
    if not grouped:
        return 0
    runs = {}
    for m in range(len(seq1)):
        runs.setdefault(seq1[m], []).append((seq2[m], pos2[m]))
    return sum(len(r) for r in runs.values()
               if len(r) > 10 and len(set(r)) < len(r))


# ---- fragments (chainvm.c:29-78) -------------------------------------------

class Frags:
    def __init__(self, kind, wf, len1, pos1, len2, pos2, distance=None):
        n = len(len1)
        self.n = n
        self.s0 = list(pos1)
        self.e0 = [pos1[i] + len1[i] - 1 for i in range(n)]
        self.s1 = list(pos2)
        self.e1 = [pos2[i] + len2[i] - 1 for i in range(n)]
        self.w = []
        for i in range(n):
            d = 0 if distance is None else distance[i]
            both = len1[i] + len2[i]
            score = both - 3 * d if d >= 0 else -(both + 3 * d)
            self.w.append(int(wf * float(abs(score))))
        if kind != GLOBAL and n > 0:
            big0, big1 = max(0, max(self.e0)), max(0, max(self.e1))
            self.ig = [pos1[i] + pos2[i] for i in range(n)]
            self.tg = [big0 - self.e0[i] + big1 - self.e1[i]
                       for i in range(n)]
        else:
            self.ig = [0] * n
            self.tg = [0] * n


def maxgap_ok(f, maxgap, left, right):
    """checkmaxgapwidth, chain2dim.c:740-774"""
    for s, e in ((f.s0[right], f.e0[left]), (f.s1[right], f.e1[left])):
        if (0 if s <= e else s - e - 1) > maxgap:
            return False
    return True


def settle(f, kind, i, j):
    """score, previous and first of fragment i with the predecessor j (or
    UNDEF): evalfragmentscore, chain2dim.c:1093-1140"""
    if j == UNDEF:
        score = f.w[i] - (f.ig[i] if kind == GLOBAL_GC else 0)
        return score, UNDEF
    score = f.score[j]
    if kind == GLOBAL:
        return score + f.w[i], j
    gc = (f.s0[i] - f.e0[j]) + (f.s1[i] - f.e1[j])
    if kind == GLOBAL_GC or score > gc:
        return score + f.w[i] - gc, j
    return f.w[i], UNDEF


def record(f, i, score, prev):
    f.score[i], f.prev[i] = score, prev
    f.first[i] = i if prev == UNDEF else f.first[prev]


def prio(f, kind, j):
    return f.score[j] - (f.tg[j] if kind != GLOBAL else 0)


def scores_sweep(f, kind, maxgap):
    """mergestartandendpoints: the fragments in the order of start1, every
    fragment activated when its end1 lies below the start at hand; the
    active ones in a list sorted by (end0, number) -> the score of the entry
    with the greatest key at the end"""
    n = f.n
    f.score, f.prev, f.first = [0] * n, [UNDEF] * n, [0] * n
    # makesortedendpointpermutation: an insertion sort, stable
    perm = sorted(range(n), key=lambda j: f.e1[j])
    tree = []

    def evaluate(i):
        j = UNDEF
        if f.s0[i] != 0:
            at = bisect.bisect_right(tree, (f.s0[i] - 1, i)) - 1
            if at >= 0:
                j = tree[at][1]
                if maxgap != 0 and not maxgap_ok(f, maxgap, j, i):
                    j = UNDEF
        record(f, i, *settle(f, kind, i, j))

    def activate(j):
        q = prio(f, kind, j)
        at = bisect.bisect_right(tree, (f.e0[j], j)) - 1
        if at < 0 or q > prio(f, kind, tree[at][1]):
            tree.insert(at + 1, (f.e0[j], j))
            while at + 2 < len(tree) and prio(f, kind, tree[at + 2][1]) < q:
                del tree[at + 2]

    s = e = 0
    while s < n and e < n:
        if f.s1[s] <= f.e1[perm[e]]:
            evaluate(s)
            s += 1
        else:
            activate(perm[e])
            e += 1
    while s < n:
        evaluate(s)
        s += 1
    while e < n:
        activate(perm[e])
        e += 1
    return f.score[tree[-1][1]]


def scores_rule(f, kind, maxgap):
    """the same scores without an order of events: the predecessor of i is,
    among the fragments j with end1[j] < start1[i] and end0[j] < start0[i],
    the one of greatest priority, ties to the smallest (end1[j], j); maxgap
    is asked of that one only -> the greatest score"""
    n = f.n
    f.score, f.prev, f.first = [0] * n, [UNDEF] * n, [0] * n
    for i in range(n):
        best = None
        for j in range(i):
            if f.e1[j] < f.s1[i] and f.s0[i] > 0 and f.e0[j] <= f.s0[i] - 1:
                k = (-prio(f, kind, j), f.e1[j], j)
                if best is None or k < best:
                    best = k
        j = UNDEF if best is None else best[2]
        if j != UNDEF and maxgap != 0 and not maxgap_ok(f, maxgap, j, i):
            j = UNDEF
        record(f, i, *settle(f, kind, i, j))
    return max(f.score)


def scores_ov(f, maxgap):
    """bruteforcechainingscores for global ov, chain2dim.c:776-888: every
    colinear fragment to the left is a candidate, maxgap is asked of each,
    the first maximum in the order of the fragments wins"""
    n = f.n
    f.score, f.prev, f.first = [0] * n, [UNDEF] * n, [0] * n
    for i in range(n):
        best = None
        for j in range(i):
            if maxgap != 0 and not maxgap_ok(f, maxgap, j, i):
                continue
            if not (f.s0[j] < f.s0[i] and f.e0[j] < f.e0[i] and
                    f.s1[j] < f.s1[i] and f.e1[j] < f.e1[i]):
                continue
            over = 0
            if f.s0[i] <= f.e0[j]:
                over += f.e0[j] - f.s0[i] + 1
            if f.s1[i] <= f.e1[j]:
                over += f.e1[j] - f.s1[i] + 1
            score = f.score[j] - over
            if score > 0:
                score, prev = score + f.w[i], j
            else:
                score, prev = f.w[i], UNDEF
            if best is None or best[0] < score:
                best = (score, prev)
        record(f, i, *(best if best is not None else (f.w[i], UNDEF)))


# ---- retrieval (chain2dim.c:1150-1360,1545-1657) ---------------------------

def right_maximal(f, i):
    """isrightmaximallocalchain: it looks at fragment i + 1 only"""
    return i == f.n - 1 or f.prev[i + 1] != i or f.score[i + 1] < f.score[i]


def retrieve(f, kind, value, globalmax):
    """-> [(score, [fragment numbers])] in the order of the last fragment"""
    n = f.n
    tgap = f.tg if kind == GLOBAL_GC else [0] * n
    ends = [i for i in range(n) if right_maximal(f, i)]
    if kind == GLOBAL:
        minscore = globalmax
    elif kind == LOCAL_THRESHOLD:
        minscore = value
    elif kind == LOCAL_BEST:
        # dictmaxsize.c keeps the `value` largest distinct keys, compared
        # as unsigned numbers
        keys = sorted({f.score[i] & MASK64 for i in ends}, reverse=True)
        worst = keys[:value][-1] if value > 0 else keys[0]
        minscore = worst - (1 << 64) if worst >> 63 else worst
    else:
        minscore = max(f.score[i] - tgap[i] for i in ends)
        if kind == LOCAL_PERCENT:
            minscore = int(float(minscore) * (1.0 - float(value) / 100.0))
    best = {}
    if kind in LOCAL_KINDS:
        for i in ends:
            c = f.first[i]
            if c not in best or best[c] < f.score[i]:
                best[c] = f.score[i]
    out = []
    for i in ends:
        s = f.score[i] - tgap[i]
        if s < minscore:
            continue
        if kind in LOCAL_KINDS:
            c = f.first[i]
            if c not in best or best[c] != s:
                continue
            del best[c]
        mem = []
        k = i
        while k != UNDEF:
            mem.append(k)
            k = f.prev[k]
        out.append((s, mem[::-1]))
    return out


def chain_problem(f, kind, value, maxgap, form="sweep"):
    """the chains of one problem -> [(score, [fragment numbers])]"""
    if f.n == 0:
        return []
    if f.n == 1:
        # chainingboundarycases, chain2dim.c:251-277
        s = f.w[0] - (f.ig[0] + f.tg[0] if kind == GLOBAL_GC else 0)
        return [(s, [0])]
    if kind == GLOBAL_OV:
        scores_ov(f, maxgap)
        top = None
    elif form == "sweep":
        top = scores_sweep(f, kind, maxgap)
    else:
        top = scores_rule(f, kind, maxgap)
    return retrieve(f, kind, value, top)


def size_classes(sizes, small=8, wave=64):
    return dict(single=sum(1 for s in sizes if s == 1),
                small=sum(1 for s in sizes if 2 <= s <= small),
                wave=sum(1 for s in sizes if small < s <= wave),
                group=sum(1 for s in sizes if s > wave))


def chain(len1, pos1, len2, pos2, seq1, seq2, kind=GLOBAL, value=0, maxgap=0,
          wf=1.0, withinborders=False, form="sweep", stable=False,
          distance=None):
    """the whole of -pp chain on a list given as what processfinal stores ->
    dict(stats, chains = rows (problem, number, score, start in members),
    members = record numbers, problems)"""
    n = len(len1)
    probs = problems(seq1, seq2, pos2, withinborders, stable)
    grouped = withinborders and len(probs) > 1
    rows, members = [], []
    for p, who in enumerate(probs):
        f = Frags(kind, wf, [len1[m] for m in who], [pos1[m] for m in who],
                  [len2[m] for m in who], [pos2[m] for m in who],
                  None if distance is None else [distance[m] for m in who])
        for c, (score, mem) in enumerate(
                chain_problem(f, kind, value, maxgap, form)):
            rows.append((p, c, score, len(members)))
            members += [who[k] for k in mem]
    sizes = [len(w) for w in probs]
    stats = dict(matches=n, problems=len(probs), largest=max(sizes, default=0),
                 tieruns=tie_runs(seq1, seq2, pos2, grouped),
                 replayed=replayed(seq1, seq2, pos2, grouped),
                 chains=len(rows), chained=len(members))
    stats.update(size_classes(sizes))
    return dict(stats=stats, chains=rows, members=members, problems=probs)


def format_chains(rows, members, lines, silent=False):
    """outvmatchchain, chainvm.c:106-161: lines[m] = the match line of
    record m without its newline"""
    out = []
    for k, (p, c, score, start) in enumerate(rows):
        end = rows[k + 1][3] if k + 1 < len(rows) else len(members)
        out.append("# chain %d: length %d score %d\n" % (c, end - start,
                                                         score))
        if not silent:
            out += [lines[m] + "\n" for m in members[start:end]]
    return "".join(out).encode()
