// Match clustering on the device: vmatch -pp matchcluster gapsize G |
// overlap P (Vmatch/clpos.c:14-201, Vmatch/matchclust.c:87-128,
// kurtz/cluster.c:458-614) on match lists that stay in HBM.  The rules --
// which pair of references is an edge between which matches -- are
// matchcluster_rules.h, the same text the host compiles.
//
//   refs     k_mc_refs, one lane per record of a list: the view of
//            select_rules.h gives length1, position1 and position2; the two
//            starts go to start[2m] and start[2m + 1], the length to
//            length[m], the record and its D/P flag are kept: the caller may
//            free the list.
//   sort     a stable radix sort of (start, index) over the significant bits
//            of the larger of the two total lengths: equal starts keep the
//            order of their index, as the reference's merging qsort does.
//   window   k_mc_window, one lane per sorted reference i: the references it
//            looks at are i + 1 .. hi_i - 1, hi_i by binary search in the
//            sorted starts (the window argument is in matchcluster_rules.h);
//            the counts hi_i - i - 1 are scanned, 64 bit.
//   pairs    one lane per CANDIDATE SLOT, not per reference: windows hold 0
//            to thousands of references, and a lane per reference would leave
//            a wavefront idle behind its largest window.  Slot s belongs to
//            the reference i with off_i <= s < off_{i+1}: k_mc_tilefirst
//            searches that i once per tile of VSA_SELECT_TILE slots, a lane
//            then searches only between the answers of its tile's ends.
//            j = i + 1 + (s - off_i).  The slots that are edges go through
//            the stable compaction of tile_compact.inc behind the edges so
//            far, as (m_i, m_j, value).  At most VSA_MATCHCLUSTER_CHUNK slots
//            per pass: the memory grows with the edges, not the candidates.
//   forest, replay, group
//            cluster_forest.inc and cluster_host.c, over the matches as
//            nodes: at most matches - 1 edges go to the host.
// The handles of vsa_eratecluster_open (erate E: the edit distance of
// the match substrings) have an edge source of their own,
// matchcluster_erate.inc; refs and everything behind the edges are shared.
// Match numbers, places of the sorted order and edge numbers are 32 bit (the
// entry points refuse more); positions, candidate counts and slot numbers
// are 64 bit.  Nothing is launched on zero elements.
#include "resident_list.hpp"
#include "matchcluster_rules.h"
#include "erate_rules.h"
#include "cluster_forest.inc"

#define MC_DEFAULT_CHUNK ((uint64_t) 1 << 26)
// every match has the references 2m and 2m + 1, and their indices are 32 bit
#define MC_MAXMATCHES ((uint64_t) 1 << 31)
enum
{
  MC_REFS,
  MC_SORT,
  MC_WINDOW,
  MC_PAIRS,
  MC_FOREST,
  MC_GROUP
};
static_assert(MC_GROUP + 1 == VSA_MATCHCLUSTER_STAGES,
              "the header counts the stages");

struct vsa_matchcluster
{
  static constexpr const char *finishname = "vsa_matchcluster_finish";
  int device = 0;
  vsa_selrules view; // the query Multiseq in device memory
  DeviceLayout layout;
  vsa_mcrules rules;
  unsigned int sortbits = 1;
  // mode VSA_MATCHCLUSTER_ERATE: the text of the index (which outlives the
  // handle) and the error rate
  const uint8_t *text = nullptr;
  uint64_t textlength = 0;
  uint32_t errorrate = 0;
  uint64_t longest = 0; // the longest match so far
  // the matches so far
  ResidentList list;
  uint64_t *start = nullptr;  // 2 per match
  uint64_t *length = nullptr; // 1 per match
  // the edges of the last finish, in the order of their numbers
  uint64_t nedges = 0;
  uint32_t *e1 = nullptr, *e2 = nullptr;
  uint64_t *value = nullptr;
  bool finished = false, grouped = false;
  vsa_clresult res;
  // ... and grouped by cluster, on the host (vsa_matchcluster_edges)
  std::vector<uint64_t> edgestart, gvalue;
  std::vector<uint32_t> g0, g1;
  // the records of the members of all clusters, in member order, on the host
  // (vsa_matchcluster_format_cluster), once per finish
  std::vector<vsa_match> memberrecs;
  bool gathered = false;
  vsa_matchclusterstats stats;
  double ms[VSA_MATCHCLUSTER_STAGES] = {0, 0, 0, 0, 0, 0};
};

namespace
{

// ---- refs -----------------------------------------------------------------------

// positions from `limit` on would not sort by the bits the sort looks at
__global__ void __launch_bounds__(TC_BLOCK)
k_mc_refs(vsa_selrules view, const vsa_match *__restrict__ in, uint64_t n,
          int palindromic, uint64_t base, uint64_t limit,
          vsa_match *__restrict__ recs, uint8_t *__restrict__ flags,
          uint64_t *__restrict__ start, uint64_t *__restrict__ length,
          unsigned long long *__restrict__ bad)
{
  const uint64_t i = vsa_bid() * TC_BLOCK + threadIdx.x;
  bool isbad = false;
  if (i < n)
  {
    const vsa_match m = in[i];
    vsa_selvalues v;
    if (vsa_sel_values(&view, &m, palindromic, &v) != 0 ||
        v.position1 >= limit || v.position2 >= limit || v.length1 >= limit)
    {
      isbad = true;
    }
    else
    {
      const uint64_t at = base + i;
      recs[at] = m;
      flags[at] = (uint8_t) (palindromic != 0);
      start[2 * at] = v.position1;
      start[2 * at + 1] = v.position2;
      length[at] = v.length1;
    }
  }
  wave_count(isbad, bad);
}

// ---- window ---------------------------------------------------------------------

// the first place of sstart[lo .. n) whose start is above x
__device__ __forceinline__ uint64_t mc_upper(const uint64_t *__restrict__ sstart,
                                             uint64_t lo, uint64_t n,
                                             uint64_t x)
{
  uint64_t hi = n;
  while (lo < hi)
  {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (sstart[mid] <= x)
    {
      lo = mid + 1;
    }
    else
    {
      hi = mid;
    }
  }
  return lo;
}

// one lane per place i of the sorted references: send[i] = the end of the
// match of reference i, count[i] = the references behind i that its loop
// looks at.  One more lane writes count[nrefs] = 0: exclusive_sum scans
// nrefs + 1 places, so that off[nrefs] is the total it fetches
__global__ void __launch_bounds__(TC_BLOCK)
k_mc_window(vsa_mcrules r, const uint64_t *__restrict__ sstart,
            const uint32_t *__restrict__ sidx,
            const uint64_t *__restrict__ length, uint64_t nrefs,
            uint64_t *__restrict__ send, uint64_t *__restrict__ count)
{
  const uint64_t i = vsa_bid() * TC_BLOCK + threadIdx.x;
  if (i > nrefs)
  {
    return;
  }
  if (i == nrefs)
  {
    count[i] = 0;
    return;
  }
  const uint64_t end = sstart[i] + length[sidx[i] >> 1];
  uint64_t c = 0;
  send[i] = end;
  if (i + 1 < nrefs && !vsa_mc_windowempty(&r, end, sstart[i + 1]))
  {
    c = mc_upper(sstart, i + 1, nrefs, vsa_mc_laststart(&r, end)) - i - 1;
  }
  count[i] = c;
}

// ---- pairs ----------------------------------------------------------------------

// the last place of off[lo .. hi] that is not above s; off[lo] <= s
__device__ __forceinline__ uint64_t mc_owner(const uint64_t *__restrict__ off,
                                             uint64_t lo, uint64_t hi,
                                             uint64_t s)
{
  while (lo < hi)
  {
    const uint64_t mid = lo + (hi - lo + 1) / 2;
    if (off[mid] <= s)
    {
      lo = mid;
    }
    else
    {
      hi = mid - 1;
    }
  }
  return lo;
}

// first[t] = the reference of the first slot of tile t of this pass;
// first[ntiles] = that of its last slot.  off[0] = 0 <= every slot.
__global__ void __launch_bounds__(TC_BLOCK)
k_mc_tilefirst(const uint64_t *__restrict__ off, uint64_t nrefs, uint64_t c0,
               uint64_t nslots, uint64_t ntiles, uint64_t *__restrict__ first)
{
  const uint64_t t = vsa_bid() * TC_BLOCK + threadIdx.x;
  if (t <= ntiles)
  {
    const uint64_t k = t * TC_TILE < nslots ? t * TC_TILE : nslots - 1;
    first[t] = mc_owner(off, 0, nrefs - 1, c0 + k);
  }
}

struct PairPayload
{
  uint32_t mi, mj;
  uint64_t value;
};

// slot k of this pass through the rules of matchcluster_rules.h
struct PairF
{
  typedef PairPayload Payload;
  vsa_mcrules r;
  const uint64_t *sstart, *send, *off, *first;
  const uint32_t *sidx;
  uint64_t c0;   // slots of the passes before
  uint64_t base; // edges of the passes before
  uint32_t *e1, *e2;
  uint64_t *value;

  __device__ int cls(uint64_t k, Payload &p) const
  {
    const uint64_t s = c0 + k, t = k / TC_TILE;
    const uint64_t i = mc_owner(off, first[t], first[t + 1], s);
    const uint64_t j = i + 1 + (s - off[i]);
    const uint64_t end_i = send[i], start_j = sstart[j];
    p.mi = sidx[i] >> 1;
    p.mj = sidx[j] >> 1;
    p.value = 0;
    return vsa_mc_classify(&r, end_i, end_i - sstart[i], p.mi, start_j,
                           send[j] - start_j, p.mj, &p.value);
  }
  __device__ void put(int, uint64_t rank, uint64_t, const Payload &p) const
  {
    e1[base + rank] = p.mi;
    e2[base + rank] = p.mj;
    value[base + rank] = p.value;
  }
};

// ---- gathers --------------------------------------------------------------------

struct EdgeGather
{
  const uint32_t *e1, *e2;
  const uint64_t *value;
  uint32_t *o1, *o2;
  uint64_t *ovalue;

  __device__ void move(uint64_t t, uint32_t i) const
  {
    o1[t] = e1[i];
    o2[t] = e2[i];
    ovalue[t] = value[i];
  }
};

// ---- host -----------------------------------------------------------------------

// the edges of one finish while they are found: a list without records
struct EdgeList
{
  uint32_t *e1 = nullptr, *e2 = nullptr;
  uint64_t *value = nullptr;
  ResidentList list;
  EdgeList()
  {
    list.records = false;
    list.column(&e1);
    list.column(&e2);
    list.column(&value);
  }
  ~EdgeList()
  {
    list.release();
  }
};

uint64_t chunkslots()
{
  const char *s = getenv("VSA_MATCHCLUSTER_CHUNK");
  if (s != nullptr && *s != '\0')
  {
    char *end = nullptr;
    const unsigned long long v = strtoull(s, &end, 10);
    if (*end == '\0' && v > 0)
    {
      return v;
    }
  }
  return MC_DEFAULT_CHUNK;
}

// sort, window, pairs: the edges of the n >= 2 matches into `edges`;
// st->candidates, samematch and below are counted
int findedges(vsa_matchcluster *c, EdgeList &edges, vsa_matchclusterstats *st,
              double *ms)
{
  const uint64_t nrefs = 2 * c->list.n;
  DevBuf idx, sidx, sstart, send, count, off;
  Timer tsort(nullptr), twindow(nullptr), tpairs(nullptr);
  if (idx.alloc(nrefs * 4) != 0 || sidx.alloc(nrefs * 4) != 0 ||
      sstart.alloc(nrefs * 8) != 0 || send.alloc(nrefs * 8) != 0 ||
      count.alloc((nrefs + 1) * 8) != 0 || off.alloc((nrefs + 1) * 8) != 0)
  {
    return -100;
  }
  tsort.start();
  k_tc_iota<<<gridfor(nrefs), TC_BLOCK, 0, nullptr>>>(idx.as<uint32_t>(),
                                                      nrefs);
  VSA_HIP(hipGetLastError());
  if (sortpairs(c->start, sstart.as<uint64_t>(), idx.as<uint32_t>(),
                sidx.as<uint32_t>(), nrefs, c->sortbits, nullptr) != 0)
  {
    return -100;
  }
  tsort.stop();
  twindow.start();
  k_mc_window<<<gridfor(nrefs + 1), TC_BLOCK, 0, nullptr>>>(
      c->rules, sstart.as<uint64_t>(), sidx.as<uint32_t>(), c->length, nrefs,
      send.as<uint64_t>(), count.as<uint64_t>());
  VSA_HIP(hipGetLastError());
  uint64_t total = 0;
  if (exclusive_sum(count.as<uint64_t>(), off.as<uint64_t>(), nrefs, nullptr,
                    &total) != 0)
  {
    return -100;
  }
  twindow.stop();
  st->candidates = total;
  tpairs.start();
  const uint64_t chunk = chunkslots();
  PairF pf;
  pf.r = c->rules;
  pf.sstart = sstart.as<uint64_t>();
  pf.send = send.as<uint64_t>();
  pf.off = off.as<uint64_t>();
  pf.sidx = sidx.as<uint32_t>();
  for (uint64_t c0 = 0; c0 < total; c0 += chunk)
  {
    const uint64_t ns = std::min<uint64_t>(chunk, total - c0),
                   nt = tilesof(ns);
    DevBuf first, offsets;
    uint64_t totals[VSA_CL_CLASSES];
    if (first.alloc((nt + 1) * 8) != 0)
    {
      return -100;
    }
    k_mc_tilefirst<<<gridfor(nt + 1), TC_BLOCK, 0, nullptr>>>(
        off.as<uint64_t>(), nrefs, c0, ns, nt, first.as<uint64_t>());
    VSA_HIP(hipGetLastError());
    pf.first = first.as<uint64_t>();
    pf.c0 = c0;
    pf.base = edges.list.n;
    pf.e1 = pf.e2 = nullptr;
    pf.value = nullptr;
    if (tc_count<1, VSA_CL_CLASSES>(pf, ns, offsets, totals) != 0)
    {
      return -100;
    }
    const uint64_t m = totals[VSA_MC_EDGE];
    st->samematch += totals[VSA_MC_SAME];
    st->below += totals[VSA_MC_BELOW];
    if (edges.list.n + m >= 0xFFFFFFFFull)
    {
      VSA_ERROR("vsa_matchcluster_finish: %lu edges: only fewer than 2^32 - 1 "
                "are covered", (unsigned long) (edges.list.n + m));
      return VSA_NOT_COVERED;
    }
    if (m > 0)
    {
      if (edges.list.reserve(edges.list.n + m) != 0)
      {
        return -100;
      }
      pf.e1 = edges.e1;
      pf.e2 = edges.e2;
      pf.value = edges.value;
      if (tc_emit<1>(pf, ns, offsets) != 0)
      {
        return -100;
      }
      edges.list.n += m;
    }
    // (first and offsets are read by the kernels of this pass)
    VSA_HIP(hipStreamSynchronize(nullptr));
  }
  tpairs.stop();
  VSA_HIP(hipStreamSynchronize(nullptr));
  ms[MC_SORT] += tsort.ms();
  ms[MC_WINDOW] += twindow.ms();
  ms[MC_PAIRS] += tpairs.ms();
  return 0;
}

#include "matchcluster_erate.inc"

// the edges grouped by cluster into host memory, once per finish
int group(vsa_matchcluster *c, const char *who)
{
  if (c->grouped)
  {
    return 0;
  }
  if (enter(c->device) != 0)
  {
    return -100;
  }
  const uint64_t ne = c->nedges, ncl = c->res.clusters;
  c->edgestart.assign(ncl + 1, 0);
  c->g0.resize(ne);
  c->g1.resize(ne);
  c->gvalue.resize(ne);
  if (ne > 0)
  {
    DevBuf order, o1, o2, ov;
    // (the span of the group stage holds cl_group's conversion of the
    // labels on the host, as that of vsa_cluster_edges does)
    Timer t(nullptr);
    t.start();
    const int rc = cl_group(c->e1, c->e2, ne, c->res.label, c->list.n, ncl, order,
                            c->edgestart, who);
    if (rc != 0)
    {
      return rc;
    }
    if (o1.alloc(ne * 4) != 0 || o2.alloc(ne * 4) != 0 ||
        ov.alloc(ne * 8) != 0)
    {
      return -100;
    }
    const EdgeGather g = {c->e1,           c->e2,           c->value,
                          o1.as<uint32_t>(), o2.as<uint32_t>(),
                          ov.as<uint64_t>()};
    k_cl_gather<EdgeGather><<<gridfor(ne), TC_BLOCK, 0, nullptr>>>(
        g, order.as<uint32_t>(), ne);
    VSA_HIP(hipGetLastError());
    t.stop();
    VSA_HIP(hipMemcpy(c->g0.data(), o1.p, ne * 4, hipMemcpyDeviceToHost));
    VSA_HIP(hipMemcpy(c->g1.data(), o2.p, ne * 4, hipMemcpyDeviceToHost));
    VSA_HIP(hipMemcpy(c->gvalue.data(), ov.p, ne * 8, hipMemcpyDeviceToHost));
    c->ms[MC_GROUP] += t.ms();
  }
  c->grouped = true;
  return 0;
}

// order[t] = the number of member t of the clusters, t < res.inclusters, in
// device memory
int memberorder(const vsa_matchcluster *c, DevBuf &order)
{
  const uint64_t k = c->res.inclusters;
  std::vector<uint32_t> h(k);
  for (uint64_t t = 0; t < k; t++)
  {
    h[t] = (uint32_t) c->res.members[t];
  }
  if (order.alloc(k * 4) != 0)
  {
    return -100;
  }
  if (k > 0)
  {
    VSA_HIP(hipMemcpy(order.p, h.data(), k * 4, hipMemcpyHostToDevice));
  }
  return 0;
}

vsa_matchcluster *newhandle(int device)
{
  vsa_matchcluster *c = new vsa_matchcluster();
  c->device = c->layout.device = c->list.device = device;
  c->list.column(&c->start, 2);
  c->list.column(&c->length);
  return c;
}

} // namespace

extern "C" void vsa_matchcluster_close(vsa_matchcluster *c)
{
  if (c == nullptr)
  {
    return;
  }
  c->layout.release();
  c->list.release();
  vsa_dev_free(c->e1);
  vsa_dev_free(c->e2);
  vsa_dev_free(c->value);
  vsa_cl_freeresult(&c->res);
  delete c;
}

extern "C" int vsa_matchcluster_open(const vsa_sinkparams *layout,
                                     const vsa_matchclusterparams *params,
                                     int device, vsa_matchcluster **cluster)
{
  if (cluster == nullptr)
  {
    VSA_ERROR("vsa_matchcluster_open: NULL argument");
    return -1;
  }
  *cluster = nullptr;
  vsa_selrules view;
  vsa_mcrules rules;
  const int rc = vsa_mc_checklayout(layout, params, "vsa_matchcluster_open",
                                    &view, &rules);
  if (rc != 0)
  {
    return rc;
  }
  if (enter(device) != 0)
  {
    return -100;
  }
  vsa_matchcluster *c = newhandle(device);
  c->view = view;
  c->rules = rules;
  memset(&c->stats, 0, sizeof c->stats);
  memset(&c->res, 0, sizeof c->res);
  c->sortbits = bitsfor(std::max(layout->totallength,
                                 layout->kind == VSA_SINK_SELF
                                     ? (uint64_t) 0
                                     : layout->querytotallength));
  if (c->layout.upload("vsa_matchcluster_open", view.nq, &c->view.qstart,
                       &c->view.qlen, 0, nullptr) != 0)
  {
    vsa_matchcluster_close(c);
    return -100;
  }
  *cluster = c;
  return 0;
}

extern "C" int vsa_eratecluster_open(const vsa_sinkparams *layout,
                                     const vsa_index *index,
                                     uint32_t errorrate, int device,
                                     vsa_matchcluster **cluster)
{
  static const char who[] = "vsa_eratecluster_open";
  if (cluster == nullptr || index == nullptr)
  {
    VSA_ERROR("%s: NULL argument", who);
    return -1;
  }
  *cluster = nullptr;
  vsa_selrules view;
  const int rc = vsa_er_checklayout(layout, errorrate, index->n, who, &view);
  if (rc != 0)
  {
    return rc;
  }
  if (index->device != device)
  {
    VSA_ERROR("%s: index on device %d, clustering on device %d", who,
              index->device, device);
    return -2;
  }
  if (enter(device) != 0)
  {
    return -100;
  }
  vsa_matchcluster *c = newhandle(device);
  c->view = view;
  c->rules.mode = VSA_MATCHCLUSTER_ERATE;
  c->rules.maxgapsize = c->rules.minpercentoverlap = 0;
  c->text = index->tis_alloc + VSA_TIS_FRONTPAD;
  c->textlength = index->n;
  c->errorrate = errorrate;
  memset(&c->stats, 0, sizeof c->stats);
  memset(&c->res, 0, sizeof c->res);
  *cluster = c;
  return 0;
}

extern "C" int vsa_matchcluster_add(vsa_matchcluster *c, const vsa_result *r,
                                    int palindromic)
{
  // the index 2m + side of a reference is 32 bit: fewer than 2^31 matches
  const int g = gate("vsa_matchcluster_add", "cluster", "clustering", c, r,
                     [&]() { return selfform(c->view.kind, palindromic); },
                     MC_MAXMATCHES, "matches: only fewer than 2^31");
  if (g != 0)
  {
    return g < 0 ? g : 0;
  }
  ScratchWords bad;
  if (c->list.reserve(c->list.n + r->count) != 0 || bad.alloc(3) != 0)
  {
    return -100;
  }
  Timer t(nullptr);
  t.start();
  if (bad.zero(0, 3) != 0)
  {
    return -100;
  }
  if (c->rules.mode == VSA_MATCHCLUSTER_ERATE)
  {
    k_er_refs<<<gridfor(r->count), TC_BLOCK, 0, nullptr>>>(
        c->view, c->text, c->textlength, r->matches, r->count, c->list.n,
        c->list.recs, c->list.flags, c->start, c->length, bad.word(0));
  } else
  {
    k_mc_refs<<<gridfor(r->count), TC_BLOCK, 0, nullptr>>>(
        c->view, r->matches, r->count, palindromic != 0, c->list.n,
        c->sortbits < 64 ? (uint64_t) 1 << c->sortbits : ~(uint64_t) 0,
        c->list.recs, c->list.flags, c->start, c->length, bad.word(0));
  }
  VSA_HIP(hipGetLastError());
  t.stop();
  // (erate: records that do not fit, records too long, the longest length)
  uint64_t bads[3] = {0, 0, 0};
  if (bad.fetch(0, 3, bads) != 0)
  {
    return -100;
  }
  const uint64_t nbad = bads[0];
  c->ms[MC_REFS] += t.ms();
  if (bads[1] != 0)
  {
    VSA_ERROR("vsa_matchcluster_add: %lu records of 2^32 symbols or more: "
              "erate covers shorter ones", (unsigned long) bads[1]);
    return VSA_NOT_COVERED;
  }
  if (nbad != 0)
  {
    return misfits("vsa_matchcluster_add", nbad,
                   c->rules.mode == VSA_MATCHCLUSTER_ERATE
                       ? "a match that leaves the text or holds a separator"
                       : "a query number outside the set, a match that leaves "
                         "its sequence or the text");
  }
  c->list.n += r->count;
  c->longest = std::max(c->longest, bads[2]);
  c->finished = false;
  return 0;
}

extern "C" int vsa_matchcluster_finish(vsa_matchcluster *c)
{
  if (c == nullptr)
  {
    VSA_ERROR("vsa_matchcluster_finish: NULL argument");
    return -1;
  }
  if (enter(c->device) != 0)
  {
    return -100;
  }
  vsa_matchclusterstats st;
  memset(&st, 0, sizeof st);
  st.matches = c->list.n;
  EdgeList edges;
  double ms[VSA_MATCHCLUSTER_STAGES] = {0, 0, 0, 0, 0, 0};
  if (c->list.n >= 2)
  {
    const int rc = c->rules.mode == VSA_MATCHCLUSTER_ERATE
                       ? findedges_erate(c, edges, &st, ms)
                       : findedges(c, edges, &st, ms);
    if (rc != 0)
    {
      return rc;
    }
  }
  std::vector<uint32_t> f1, f2;
  uint64_t changed = 0;
  if (edges.list.n > 0)
  {
    Timer t(nullptr);
    t.start();
    const int rc = cl_forest(c->list.n, edges.e1, edges.e2, edges.list.n, f1, f2,
                             &st.rounds, "vsa_matchcluster_finish");
    if (rc != 0)
    {
      return rc;
    }
    t.stop();
    VSA_HIP(hipStreamSynchronize(nullptr));
    ms[MC_FOREST] += t.ms();
  }
  vsa_clresult res;
  const int rc = vsa_cl_replay(c->list.n, f1.data(), f2.data(), f1.size(), &changed,
                               &res);
  if (rc != 0)
  {
    return rc;
  }
  if (changed != f1.size())
  {
    VSA_ERROR("vsa_matchcluster_finish: only %lu of the %lu forest edges "
              "joined two clusters", (unsigned long) changed,
              (unsigned long) f1.size());
    vsa_cl_freeresult(&res);
    return -101;
  }
  // from here on nothing fails: the state changes
  vsa_dev_free(c->e1);
  vsa_dev_free(c->e2);
  vsa_dev_free(c->value);
  c->e1 = edges.e1;
  c->e2 = edges.e2;
  c->value = edges.value;
  c->nedges = edges.list.n;
  edges.e1 = edges.e2 = nullptr;
  edges.value = nullptr;
  vsa_cl_freeresult(&c->res);
  c->res = res;
  st.edges = c->nedges;
  st.forestedges = f1.size();
  st.clusters = res.clusters;
  st.inclusters = res.inclusters;
  c->stats = st;
  for (int q = 0; q < VSA_MATCHCLUSTER_STAGES; q++)
  {
    c->ms[q] += ms[q];
  }
  c->finished = true;
  c->grouped = false;
  c->gathered = false;
  return 0;
}

extern "C" int vsa_matchcluster_getstats(const vsa_matchcluster *c,
                                         vsa_matchclusterstats *stats)
{
  if (c == nullptr || stats == nullptr)
  {
    VSA_ERROR("vsa_matchcluster_getstats: NULL argument");
    return -1;
  }
  *stats = c->stats;
  return 0;
}

extern "C" int vsa_matchcluster_members(const vsa_matchcluster *c,
                                        uint64_t *clusterstart,
                                        uint64_t *members)
{
  const int rc = needfinished(c, "vsa_matchcluster_members");
  if (rc != 0)
  {
    return rc;
  }
  if (clusterstart != nullptr)
  {
    memcpy(clusterstart, c->res.clusterstart, (c->res.clusters + 1) * 8);
  }
  if (members != nullptr && c->res.inclusters > 0)
  {
    memcpy(members, c->res.members, c->res.inclusters * 8);
  }
  return 0;
}

extern "C" int vsa_matchcluster_labels(const vsa_matchcluster *c,
                                       uint64_t *label)
{
  const int rc = needfinished(c, "vsa_matchcluster_labels");
  if (rc != 0)
  {
    return rc;
  }
  if (label == nullptr)
  {
    VSA_ERROR("vsa_matchcluster_labels: NULL argument");
    return -1;
  }
  if (c->list.n > 0)
  {
    memcpy(label, c->res.label, c->list.n * 8);
  }
  return 0;
}

extern "C" int vsa_matchcluster_edges(vsa_matchcluster *c, uint64_t *edgestart,
                                      uint32_t *m0, uint32_t *m1,
                                      uint64_t *value)
{
  int rc = needfinished(c, "vsa_matchcluster_edges");
  if (rc != 0 || (rc = group(c, "vsa_matchcluster_edges")) != 0)
  {
    return rc;
  }
  const uint64_t ne = c->nedges;
  if (edgestart != nullptr)
  {
    memcpy(edgestart, c->edgestart.data(), (c->res.clusters + 1) * 8);
  }
  if (m0 != nullptr && ne > 0)
  {
    memcpy(m0, c->g0.data(), ne * 4);
  }
  if (m1 != nullptr && ne > 0)
  {
    memcpy(m1, c->g1.data(), ne * 4);
  }
  if (value != nullptr && ne > 0)
  {
    memcpy(value, c->gvalue.data(), ne * 8);
  }
  return 0;
}

extern "C" int vsa_matchcluster_records(vsa_matchcluster *c,
                                        vsa_result **records,
                                        uint8_t *palindromic)
{
  const int rc = needfinished(c, "vsa_matchcluster_records");
  if (rc != 0)
  {
    return rc;
  }
  if (records == nullptr)
  {
    VSA_ERROR("vsa_matchcluster_records: NULL argument");
    return -1;
  }
  *records = nullptr;
  DevBuf order;
  if (enter(c->device) != 0 || memberorder(c, order) != 0)
  {
    return -100;
  }
  return records_of(c->list, order.as<uint32_t>(), c->res.inclusters,
                    palindromic, nullptr, records);
}

extern "C" int64_t vsa_matchcluster_format(const vsa_matchcluster *c,
                                           char *buffer, uint64_t capacity)
{
  const int rc = needfinished(c, "vsa_matchcluster_format");
  if (rc != 0)
  {
    return rc;
  }
  if (buffer == nullptr)
  {
    VSA_ERROR("vsa_matchcluster_format: NULL argument");
    return -1;
  }
  return vsa_mc_format(c->list.n, &c->res, buffer, capacity);
}

extern "C" int64_t vsa_matchcluster_format_cluster(vsa_matchcluster *c,
                                                   vsa_sink *sink,
                                                   uint64_t cnum, char *buffer,
                                                   uint64_t capacity)
{
  int rc = needfinished(c, "vsa_matchcluster_format_cluster");
  if (rc != 0)
  {
    return rc;
  }
  if (sink == nullptr || buffer == nullptr)
  {
    VSA_ERROR("vsa_matchcluster_format_cluster: NULL argument");
    return -1;
  }
  if (cnum >= c->res.clusters)
  {
    VSA_ERROR("vsa_matchcluster_format_cluster: cluster %lu of %lu",
              (unsigned long) cnum, (unsigned long) c->res.clusters);
    return -2;
  }
  if ((rc = group(c, "vsa_matchcluster_format_cluster")) != 0)
  {
    return rc;
  }
  if (enter(c->device) != 0)
  {
    return -100;
  }
  const uint64_t first = c->res.clusterstart[cnum],
                 size = c->res.clusterstart[cnum + 1] - first,
                 e0 = c->edgestart[cnum], ne = c->edgestart[cnum + 1] - e0;
  if (!c->gathered)
  {
    // the records of all members into host memory, once per finish
    DevBuf order;
    if (memberorder(c, order) != 0 ||
        members_to_host(c->list, order.as<uint32_t>(), c->res.inclusters,
                        c->memberrecs) != 0)
    {
      return -100;
    }
    c->gathered = true;
  }
  return vsa_matchcluster_format_host(
      sink, c->rules.mode, c->res.members + first,
      c->memberrecs.data() + first, size,
      c->g0.data() + e0, c->g1.data() + e0, c->gvalue.data() + e0, ne, buffer,
      capacity);
}

extern "C" int vsa_matchcluster_times(const vsa_matchcluster *c, double *ms)
{
  if (c == nullptr || ms == nullptr)
  {
    VSA_ERROR("vsa_matchcluster_times: NULL argument");
    return -1;
  }
  memcpy(ms, c->ms, sizeof c->ms);
  return 0;
}
