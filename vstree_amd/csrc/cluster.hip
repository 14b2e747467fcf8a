// Sequence clustering on the device: vmatch -dbcluster percsmall perclarge
// (Vmatch/vmcluster.c:289-415, kurtz/cluster.c:436-614) on match lists that
// stay in HBM.  The rules -- which record is an edge between which sequences
// -- are cluster_rules.h, the same text the host compiles.
//
//   edges    one lane per record, tiles of VSA_SELECT_TILE records: the two
//            sequences by binary search in markpos, the overlap test.  The
//            accepted records go through the stable compaction of
//            tile_compact.inc behind the edges of the lists added before.
//            An edge keeps its record and its D/P flag: the caller may free
//            the list.
//   forest   linkcluster is sequential, but an edge changes its state only if
//            its ends are in different clusters at that moment: those edges
//            are the minimum spanning forest of the list with weight = edge
//            number (Kruskal takes exactly them).  Boruvka finds the same
//            forest in rounds: every live edge looks up the roots of its
//            ends; equal roots: the edge is dead; else a 64-bit atomicMin of
//            its number into best[] of both roots.  Every root with a best
//            edge marks it and hooks itself to the other root; where two
//            roots chose the same edge only the larger one hooks.  Weights
//            are distinct, so no other cycle arises.  The hooks go into a
//            second parent array (no lane reads what another one writes in
//            the same kernel), pointer jumping flattens it.  At most
//            VSA_CLUSTER_MAXROUNDS rounds and VSA_CLUSTER_MAXJUMPS jumps per
//            round, an error beyond; no loop waits for another lane.
//   replay   the forest edges, compacted in the order of their numbers (at
//            most numofsequences - 1), go to the host: cluster_host.c sends
//            them through linkcluster and numbers the clusters.
//   group    vsa_cluster_edges: every edge is keyed by the cluster of its
//            sequences; a stable radix sort of the edges in reverse order
//            puts each cluster's edges together in descending number, the
//            order addClusterEdge leaves them in.
// Sequence and edge numbers are 32 bit (the entry points refuse more),
// positions and record indices 64 bit.
#include "search_host.hpp"
#include "cluster_rules.h"
#include "cluster_forest.inc"

struct vsa_cluster
{
  int device = 0;
  int kind = 0;
  vsa_clrules rules; // markpos in device memory
  uint64_t *d_markpos = nullptr;
  // the edges so far
  uint64_t nedges = 0, capacity = 0;
  uint32_t *e1 = nullptr, *e2 = nullptr;
  vsa_match *recs = nullptr;
  uint8_t *flags = nullptr;
  bool finished = false;
  vsa_clresult res;
  vsa_clusterstats stats;
  double add_ms = 0, finish_ms = 0, edges_ms = 0;
};

namespace
{

struct EdgePayload
{
  uint32_t s1, s2;
};

// a record through the rules of cluster_rules.h
struct EdgeF
{
  typedef EdgePayload Payload;
  vsa_clrules r;
  const vsa_match *matches;
  int palindromic;
  uint64_t base; // edges of the lists before
  uint32_t *e1, *e2;
  vsa_match *recs;
  uint8_t *flags;

  __device__ int cls(uint64_t i, Payload &p) const
  {
    const vsa_match m = matches[i];
    uint64_t s1 = 0, s2 = 0;
    const int c = vsa_cl_classify(&r, &m, palindromic, &s1, &s2);
    p.s1 = (uint32_t) s1;
    p.s2 = (uint32_t) s2;
    return c;
  }
  __device__ void put(int, uint64_t rank, uint64_t i, const Payload &p) const
  {
    e1[base + rank] = p.s1;
    e2[base + rank] = p.s2;
    recs[base + rank] = matches[i];
    flags[base + rank] = (uint8_t) (palindromic != 0);
  }
};

// room for `need` edges; what is there stays.  Array by array (one wait
// each, the old and the new block of one array at a time): where a later one
// fails, the earlier ones are larger than `capacity` says, which stays right
int reserve(vsa_cluster *c, uint64_t need)
{
  if (need <= c->capacity)
  {
    return 0;
  }
  const uint64_t cap = std::max<uint64_t>(need, 2 * c->capacity);
  if (grow((void **) &c->e1, c->nedges, cap, 4) != 0 ||
      grow((void **) &c->e2, c->nedges, cap, 4) != 0 ||
      grow((void **) &c->recs, c->nedges, cap, sizeof(vsa_match)) != 0 ||
      grow((void **) &c->flags, c->nedges, cap, 1) != 0)
  {
    return -100;
  }
  c->capacity = cap;
  return 0;
}

} // namespace

extern "C" void vsa_cluster_close(vsa_cluster *c)
{
  if (c == nullptr)
  {
    return;
  }
  (void) hipSetDevice(c->device);
  (void) hipFree(c->d_markpos);
  vsa_dev_free(c->e1);
  vsa_dev_free(c->e2);
  vsa_dev_free(c->recs);
  vsa_dev_free(c->flags);
  vsa_cl_freeresult(&c->res);
  delete c;
}

extern "C" int vsa_cluster_open(const vsa_sinkparams *layout,
                                const vsa_clusterparams *params, int device,
                                vsa_cluster **cluster)
{
  if (cluster == nullptr)
  {
    VSA_ERROR("vsa_cluster_open: NULL argument");
    return -1;
  }
  *cluster = nullptr;
  const int rc = vsa_cl_checklayout(layout, params, "vsa_cluster_open");
  if (rc != 0)
  {
    return rc;
  }
  if (enter(device) != 0)
  {
    return -100;
  }
  vsa_cluster *c = new vsa_cluster();
  c->device = device;
  c->kind = layout->kind;
  memset(&c->stats, 0, sizeof c->stats);
  memset(&c->res, 0, sizeof c->res);
  const uint64_t nmark = layout->numofsequences - 1;
  if (vsa_hip_malloc((void **) &c->d_markpos, nmark * 8) != hipSuccess ||
      hipMemcpy(c->d_markpos, layout->markpos, nmark * 8,
                hipMemcpyHostToDevice) != hipSuccess)
  {
    VSA_ERROR("vsa_cluster_open: upload of the separator positions failed");
    vsa_cluster_close(c);
    return -100;
  }
  c->rules.totallength = layout->totallength;
  c->rules.numofsequences = layout->numofsequences;
  c->rules.markpos = c->d_markpos;
  c->rules.percsmall = params->percsmall;
  c->rules.perclarge = params->perclarge;
  *cluster = c;
  return 0;
}

extern "C" int vsa_cluster_add(vsa_cluster *c, const vsa_result *r,
                               int palindromic)
{
  if (c == nullptr || r == nullptr)
  {
    VSA_ERROR("vsa_cluster_add: NULL argument");
    return -1;
  }
  if (r->packbits != 0)
  {
    VSA_ERROR("vsa_cluster_add: a packed candidate result has no records to "
              "cluster by");
    return VSA_NOT_COVERED;
  }
  if (!palindromic && c->kind != VSA_SINK_SELF)
  {
    VSA_ERROR("vsa_cluster_add: a direct list, the layout is that of vmatch "
              "-p IDX");
    return VSA_NOT_COVERED;
  }
  if (r->device != c->device)
  {
    VSA_ERROR("vsa_cluster_add: result on device %d, clustering on device %d",
              r->device, c->device);
    return -2;
  }
  if (enter(c->device) != 0)
  {
    return -100;
  }
  if (r->count == 0)
  {
    return 0;
  }
  Timer t(nullptr);
  t.start();
  EdgeF ef;
  ef.r = c->rules;
  ef.matches = r->matches;
  ef.palindromic = palindromic != 0;
  ef.base = c->nedges;
  ef.e1 = ef.e2 = nullptr;
  ef.recs = nullptr;
  ef.flags = nullptr;
  DevBuf offsets;
  uint64_t totals[VSA_CL_CLASSES];
  if (tc_count<1, VSA_CL_CLASSES>(ef, r->count, offsets, totals) != 0)
  {
    return -100;
  }
  if (totals[VSA_CL_BAD] != 0)
  {
    VSA_ERROR("vsa_cluster_add: %lu records do not fit the layout (a match "
              "that leaves its sequence, or a sequence number outside the %lu "
              "of the index)", (unsigned long) totals[VSA_CL_BAD],
              (unsigned long) c->rules.numofsequences);
    return -2;
  }
  const uint64_t m = totals[VSA_CL_EDGE];
  if (c->nedges + m >= 0xFFFFFFFFull)
  {
    VSA_ERROR("vsa_cluster_add: %lu edges: only fewer than 2^32 - 1 are "
              "covered", (unsigned long) (c->nedges + m));
    return VSA_NOT_COVERED;
  }
  if (m > 0)
  {
    int rc = reserve(c, c->nedges + m);
    if (rc != 0)
    {
      return rc;
    }
    ef.e1 = c->e1;
    ef.e2 = c->e2;
    ef.recs = c->recs;
    ef.flags = c->flags;
    if (tc_emit<1>(ef, r->count, offsets) != 0)
    {
      return -100;
    }
  }
  t.stop();
  VSA_HIP(hipStreamSynchronize(nullptr));
  c->add_ms += t.ms();
  c->nedges += m;
  c->finished = false;
  c->stats.seen += r->count;
  c->stats.samesequence += totals[VSA_CL_SAME];
  c->stats.mirrordropped += totals[VSA_CL_MIRROR];
  c->stats.rejected += totals[VSA_CL_REJECTED];
  c->stats.edges = c->nedges;
  return 0;
}

extern "C" int vsa_cluster_finish(vsa_cluster *c)
{
  if (c == nullptr)
  {
    VSA_ERROR("vsa_cluster_finish: NULL argument");
    return -1;
  }
  if (enter(c->device) != 0)
  {
    return -100;
  }
  std::vector<uint32_t> f1, f2;
  uint64_t rounds = 0, changed = 0;
  Timer t(nullptr);
  t.start();
  if (c->nedges > 0)
  {
    const int rc = cl_forest(c->rules.numofsequences, c->e1, c->e2, c->nedges,
                             f1, f2, &rounds, "vsa_cluster_finish");
    if (rc != 0)
    {
      return rc;
    }
  }
  t.stop();
  VSA_HIP(hipStreamSynchronize(nullptr));
  c->finish_ms += t.ms();
  vsa_clresult res;
  const int rc = vsa_cl_replay(c->rules.numofsequences, f1.data(), f2.data(),
                               f1.size(), &changed, &res);
  if (rc != 0)
  {
    return rc;
  }
  if (changed != f1.size())
  {
    VSA_ERROR("vsa_cluster_finish: only %lu of the %lu forest edges joined "
              "two clusters", (unsigned long) changed,
              (unsigned long) f1.size());
    vsa_cl_freeresult(&res);
    return -101;
  }
  vsa_cl_freeresult(&c->res);
  c->res = res;
  c->finished = true;
  c->stats.forestedges = f1.size();
  c->stats.rounds = rounds;
  c->stats.clusters = res.clusters;
  c->stats.inclusters = res.inclusters;
  c->stats.singlets = res.numofsequences - res.inclusters;
  return 0;
}

extern "C" int vsa_cluster_getstats(const vsa_cluster *c,
                                    vsa_clusterstats *stats)
{
  if (c == nullptr || stats == nullptr)
  {
    VSA_ERROR("vsa_cluster_getstats: NULL argument");
    return -1;
  }
  *stats = c->stats;
  return 0;
}

static int needfinished(const vsa_cluster *c, const char *who)
{
  if (c == nullptr)
  {
    VSA_ERROR("%s: NULL argument", who);
    return -1;
  }
  if (!c->finished)
  {
    VSA_ERROR("%s: vsa_cluster_finish has not seen the last list", who);
    return -2;
  }
  return 0;
}

extern "C" int vsa_cluster_members(const vsa_cluster *c,
                                   uint64_t *clusterstart, uint64_t *members)
{
  const int rc = needfinished(c, "vsa_cluster_members");
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

extern "C" int vsa_cluster_labels(const vsa_cluster *c, uint64_t *label)
{
  const int rc = needfinished(c, "vsa_cluster_labels");
  if (rc != 0)
  {
    return rc;
  }
  if (label == nullptr)
  {
    VSA_ERROR("vsa_cluster_labels: NULL argument");
    return -1;
  }
  memcpy(label, c->res.label, c->res.numofsequences * 8);
  return 0;
}

extern "C" int64_t vsa_cluster_format(const vsa_cluster *c, char *buffer,
                                      uint64_t capacity)
{
  const int rc = needfinished(c, "vsa_cluster_format");
  if (rc != 0)
  {
    return rc;
  }
  if (buffer == nullptr)
  {
    VSA_ERROR("vsa_cluster_format: NULL argument");
    return -1;
  }
  return vsa_cl_format(&c->res, buffer, capacity);
}

extern "C" int vsa_cluster_times(const vsa_cluster *c, double *add_ms,
                                 double *finish_ms, double *edges_ms)
{
  if (c == nullptr || add_ms == nullptr || finish_ms == nullptr ||
      edges_ms == nullptr)
  {
    VSA_ERROR("vsa_cluster_times: NULL argument");
    return -1;
  }
  *add_ms = c->add_ms;
  *finish_ms = c->finish_ms;
  *edges_ms = c->edges_ms;
  return 0;
}

extern "C" int vsa_cluster_edges(vsa_cluster *c, vsa_result **edges,
                                 uint8_t *palindromic, uint64_t *edgestart)
{
  int rc = needfinished(c, "vsa_cluster_edges");
  if (rc != 0)
  {
    return rc;
  }
  if (edges == nullptr)
  {
    VSA_ERROR("vsa_cluster_edges: NULL argument");
    return -1;
  }
  *edges = nullptr;
  if (enter(c->device) != 0)
  {
    return -100;
  }
  const uint64_t ne = c->nedges, nseq = c->rules.numofsequences,
                 ncl = c->res.clusters;
  vsa_result *res = newresult(c->device);
  if (ne == 0)
  {
    if (edgestart != nullptr)
    {
      edgestart[0] = 0;
    }
    *edges = res;
    return 0;
  }
  ResultGuard guard = {res};
  Timer t(nullptr);
  t.start();
  DevBuf order, oflags;
  std::vector<uint64_t> hstart;
  if (oflags.alloc(ne) != 0 ||
      vsa_dev_alloc((void **) &res->matches, ne * sizeof(vsa_match)) != 0)
  {
    return -100;
  }
  rc = cl_group(c->e1, c->e2, ne, c->res.label, nseq, ncl, order, hstart,
                "vsa_cluster_edges");
  if (rc != 0)
  {
    return rc;
  }
  const RecGather g = {c->recs, c->flags, res->matches, oflags.as<uint8_t>()};
  k_cl_gather<RecGather><<<gridfor(ne), TC_BLOCK, 0, nullptr>>>(
      g, order.as<uint32_t>(), ne);
  VSA_HIP(hipGetLastError());
  t.stop();
  VSA_HIP(hipStreamSynchronize(nullptr));
  c->edges_ms += t.ms();
  if (palindromic != nullptr)
  {
    VSA_HIP(hipMemcpy(palindromic, oflags.p, ne, hipMemcpyDeviceToHost));
  }
  if (edgestart != nullptr)
  {
    memcpy(edgestart, hstart.data(), (ncl + 1) * 8);
  }
  res->count = ne;
  res->stats.count = ne;
  if (sumlengths(res->matches, ne, nullptr, &res->stats.sumlength) != 0)
  {
    return -100;
  }
  guard.r = nullptr;
  *edges = res;
  return 0;
}
