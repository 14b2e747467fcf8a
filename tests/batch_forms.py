"""The forms in which a batch of reads reaches the seed extensions and the
alignment -- ragged and uniform byte batches, reads at two bits per symbol,
dense device memory, each with a sequence offset -- and the hand-made
scenarios of extend_cases.py, extend_edist_cases.py, extend_xdrop_cases.py
and align_cases.py with their reads padded to one length, so that every form
can hold them.  Shared by test_batch_forms_host.py (what can be checked
without a GPU) and test_gpu_degenerate_forms.py."""
import copy

import numpy as np

import align_cases as AC
import extend_cases as EC
import extend_edist_cases as DC
import extend_edist_model as DM
import extend_model as EM
import extend_xdrop_cases as XC
import extend_xdrop_model as XM
import helpers as H

SEP, WILD = H.SEPARATOR, H.WILDCARD

# the limits the library exports (test_extend_refusals.py pins them)
LANE_BUDGET, LONG_STEP = 256, 1024

FORMS = ("ragged", "uniform", "packed", "dense")
# no offset, the smallest, one whose sum with a sequence number needs 33 bits
OFFSETS = (0, 1, (1 << 32) + 5)

# (entry, scenario): what runs through which entry
CASES = [("hamming", "borders_dense"), ("hamming", "specials"),
         ("edist", "borders_dense"), ("edist", "specials"),
         ("edist", "indels"),
         ("xdrop", "borders_dense"), ("xdrop", "hspecials"),
         ("xdrop", "indels"), ("xdrop", "mirrored"),
         ("align", "distance1"), ("align", "distance8"),
         ("align", "distance16"), ("align", "mixed")]


def case_id(case):
    return "%s-%s" % case


# --------------------------------------------------------------------------
# reads of one length
# --------------------------------------------------------------------------

def reads_of(sc):
    """the reads of a scenario of any of the four modules as arrays"""
    return [np.asarray(r[1] if isinstance(r, tuple) else r, np.uint8)
            for r in sc.reads]


def common_length(reads):
    """the smallest length all reads can be given that is no multiple of 4
    (nor, then, of 32): a row of packed reads ends inside a byte"""
    m = max(len(r) for r in reads)
    return m if m % 4 else m + 1


def padded(sc, how):
    """a copy of `sc` whose reads are filled up behind to common_length.
    how == "sep": a separator, then symbols -- what stands behind a read in
    the query Multiseq anyway, so every list stays what it is; but a read
    with a separator has no reverse complement, and a packed batch keeps it
    in its side list.  how == "plain": symbols of the alphabet, and a
    wildcard at the end of the first read that is filled up: the extensions
    may run into them, so the lists are those of the model on THIS batch."""
    assert how in ("sep", "plain")
    reads = reads_of(sc)
    m = common_length(reads)
    rng = np.random.default_rng(4242)
    new, marked = [], False
    for r in reads:
        fill = rng.integers(0, 4, m - len(r)).astype(np.uint8)
        if len(fill) and how == "sep":
            fill[0] = SEP
        elif len(fill) and not marked:
            fill[-1] = WILD
            marked = True
        new.append(np.concatenate((r, fill)))
    out = copy.copy(sc)
    if isinstance(sc.reads[0], tuple):
        out.reads = [(w, r) for (w, _), r in zip(sc.reads, new)]
    else:
        out.reads = new
    if hasattr(sc, "dense"):
        out.dense = False       # separators between the reads
    out.name = "%s+%s" % (sc.name, how)
    return out


def may_reverse(sc):
    """readmulti.c:45-49: the reverse complement of a separator is undefined"""
    return not any((r == SEP).any() for r in reads_of(sc))


def as_palindromic(sc):
    """an align_cases.Planted whose reads are stored as their reverse
    complements: the forward batch of a palindromic list of the same records"""
    out = copy.copy(sc)
    out.palindromic = True
    out.reads = [AC.rc(r) for r in sc.reads]
    out.name = sc.name + "+p"
    return out


def block_of(q):
    """the reads of a batch of one length back to back -> (symbols, m)"""
    m = int(q.length[0])
    assert (q.length == m).all()
    return np.concatenate([q.seq(i) for i in range(q.nq)]), m


def in_side_list(q):
    """how many reads a packed batch keeps as bytes"""
    return sum(1 for i in range(q.nq) if (q.seq(i) > 3).any())


def device_batch(V, q, form, offset=0):
    """the batch `q` (H.Queries) on the device in one of FORMS"""
    if form in ("ragged", "uniform"):
        assert form == "ragged" or len(set(q.length.tolist())) == 1
        gq = V.Queries.from_host(q.symbols, q.start, q.length)
    else:
        block, m = block_of(q)
        if form == "packed":
            assert m % 4 != 0 and in_side_list(q) > 0
            gq = V.Queries.from_host_packed(block, m)
        else:
            d = V.device_malloc(len(block))
            try:
                V.device_upload(d, block)
                gq = V.Queries.from_device(d, q.nq, m)
            finally:
                V.device_free(d)
    assert gq.nq == q.nq
    if offset:
        gq.set_offset(offset)
    assert gq.info().offset == offset
    return gq


def shifted(rec, k):
    out = np.array(rec, H.MATCH_DTYPE)
    out["queryseq"] += np.uint64(k)
    return out


# --------------------------------------------------------------------------
# the scenarios and their models, made once
# --------------------------------------------------------------------------

_scenarios = {}
_models = {}


def scenario(case, how=None):
    """the scenario of a case; how: with its reads padded"""
    if not _scenarios:
        for name, sc in EC.scenarios(LANE_BUDGET, LONG_STEP).items():
            _scenarios["hamming", name, None] = sc
        for name, sc in DC.scenarios(LANE_BUDGET).items():
            _scenarios["edist", name, None] = sc
        for name, sc in XC.scenarios(LANE_BUDGET, LONG_STEP).items():
            _scenarios["xdrop", name, None] = sc
        for D in (1, 8, 16):       # one per group width: 16, 32 and 64 lanes
            _scenarios["align", "distance%d" % D, None] = \
                AC.planted_distance(D)
        _scenarios["align", "mixed", None] = AC.planted_mixed(AC.QUERY_EDIST)
    k = case + (how,)
    if k not in _scenarios:
        _scenarios[k] = padded(_scenarios[case + (None,)], how)
    return _scenarios[k]


def params(case):
    """the parameter sets of a case"""
    entry, sc = case[0], scenario(case)
    if entry == "align":
        return [()]
    return XC.modes(sc) if entry == "xdrop" else list(sc.params)


def model(case, how, p, palindromic=False):
    """the list of the model: records, or (offsets, words) for align --
    computed once, shared, left unchanged"""
    k = (case, how, p, bool(palindromic) and case[0] == "align")
    if k not in _models:
        sc = scenario(case, how)
        if case[0] == "align":
            got = (as_palindromic(sc) if palindromic else sc).model()
            for a in got:
                a.setflags(write=False)
        else:
            got = sc.model(*p)
            got.setflags(write=False)
        _models[k] = got
    return _models[k]


def distances(case, p, rec):
    """the distances of extended seeds"""
    return {"hamming": EM.distances, "edist": DM.distances,
            "xdrop": XM.distances}[case[0]](rec)


def forward_batch(case, how, palindromic):
    """the batch the caller holds: for a palindromic list the reverse
    complement of the scenario's"""
    sc = scenario(case, how)
    if not palindromic:
        return sc.queries()
    assert may_reverse(sc)
    if case[0] == "align":
        return as_palindromic(sc).queries()
    return EC.reverse_complement(sc.queries())


def pads(form, palindromic):
    """how the reads of a form are filled up: the ragged batch is the
    scenario as it is; a direct pass takes both paddings, a palindromic one
    has no separators to offer"""
    if form == "ragged":
        return (None,)
    return ("plain",) if palindromic else ("sep", "plain")


def border_records(case):
    """the records of the first and of the last read of a scenario"""
    sc = scenario(case)
    rec, nq = sc.records(), sc.queries().nq
    out = np.concatenate((rec[rec["queryseq"] == 0],
                          rec[rec["queryseq"] == nq - 1]))
    assert nq > 1 and {0, nq - 1} == set(out["queryseq"].tolist())
    return out


# --------------------------------------------------------------------------
# a query file in three batches (test_gpu_degenerate_chain.py)
# --------------------------------------------------------------------------

# case -> the cuts: a batch of one read, no cut at a multiple of 64, and
# reads with matches on both sides of a cut
CUTS = {"c6": (113, 114), "micro": (1, 6)}
# (case, mode) -> (L, K, the recorded -s run, the recorded run of the
# extension) -- of the latter two what exists
PIECED = {("c6", "e"): (25, 2, "c6_q_l25_e2_dp_s40", None),
          ("c6", "h"): (20, 2, "c6_q_l20_h2_dp_s", None),
          ("micro", "e"): (8, 1, "micro_q_l8_e1_s30", "micro_q_l8_e1"),
          ("micro", "h"): (8, 1, None, "micro_q_l8_h1")}


def pieces(case):
    """[(first read, behind the last read)] of the three batches"""
    _, q = AC.load(case)
    a, b = CUTS[case]
    return [(0, a), (a, b), (b, len(q.length))]


def beside_cuts(case):
    """the reads on both sides of a cut that must have matches; of micro's
    eight reads only 0 and 1 are neighbours with matches"""
    a, b = CUTS[case]
    return (a - 1, a, b - 1, b) if case != "micro" else (a - 1, a)


def recorded_reads(case, mode):
    """the reads with a direct match in the recorded runs of a pieced case"""
    _, _, skey, ekey = PIECED[case, mode]
    out = []
    if skey is not None:
        rows = AC.expected(skey, "rows")
        out.append(set(rows[rows[:, 7] == 0][:, 4].tolist()))
    if ekey is not None and mode == "e":
        rows = DC.expected_rows(ekey)
        out.append(set(rows[rows[:, 7] == 0][:, 4].tolist()))
    if ekey is not None and mode == "h":
        rows = EC.expected_rows(ekey)
        out.append(set(rows[rows[:, 6] == 0][:, 3].tolist()))
    assert all(x == out[0] for x in out)
    return out[0]
