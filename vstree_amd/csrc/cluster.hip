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
#include "resident_list.hpp"
#include "cluster_rules.h"
#include "cluster_forest.inc"

struct vsa_cluster
{
  static constexpr const char *finishname = "vsa_cluster_finish";
  int device = 0;
  int kind = 0;
  vsa_clrules rules; // markpos in device memory
  DeviceLayout layout;
  // the edges so far: their records and flags, and their ends
  ResidentList list;
  uint32_t *e1 = nullptr, *e2 = nullptr;
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

} // namespace

extern "C" void vsa_cluster_close(vsa_cluster *c)
{
  if (c == nullptr)
  {
    return;
  }
  c->layout.release();
  c->list.release();
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
  c->device = c->layout.device = c->list.device = device;
  c->list.column(&c->e1);
  c->list.column(&c->e2);
  c->kind = layout->kind;
  memset(&c->stats, 0, sizeof c->stats);
  memset(&c->res, 0, sizeof c->res);
  c->rules.markpos = layout->markpos;
  if (c->layout.upload("vsa_cluster_open", 0, nullptr, nullptr,
                       layout->numofsequences - 1, &c->rules.markpos) != 0)
  {
    vsa_cluster_close(c);
    return -100;
  }
  c->rules.totallength = layout->totallength;
  c->rules.numofsequences = layout->numofsequences;
  c->rules.percsmall = params->percsmall;
  c->rules.perclarge = params->perclarge;
  *cluster = c;
  return 0;
}

extern "C" int vsa_cluster_add(vsa_cluster *c, const vsa_result *r,
                               int palindromic)
{
  // (the edges are counted below: their limit is not the gate's)
  const int g = gate("vsa_cluster_add", "cluster by", "clustering", c, r,
                     [&]() {
                       return !palindromic && c->kind != VSA_SINK_SELF
                                  ? "a direct list, the layout is that of "
                                    "vmatch -p IDX"
                                  : nullptr;
                     },
                     0, nullptr);
  if (g != 0)
  {
    return g < 0 ? g : 0;
  }
  Timer t(nullptr);
  t.start();
  EdgeF ef;
  ef.r = c->rules;
  ef.matches = r->matches;
  ef.palindromic = palindromic != 0;
  ef.base = c->list.n;
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
  if (c->list.n + m >= 0xFFFFFFFFull)
  {
    VSA_ERROR("vsa_cluster_add: %lu edges: only fewer than 2^32 - 1 are "
              "covered", (unsigned long) (c->list.n + m));
    return VSA_NOT_COVERED;
  }
  if (m > 0)
  {
    int rc = c->list.reserve(c->list.n + m);
    if (rc != 0)
    {
      return rc;
    }
    ef.e1 = c->e1;
    ef.e2 = c->e2;
    ef.recs = c->list.recs;
    ef.flags = c->list.flags;
    if (tc_emit<1>(ef, r->count, offsets) != 0)
    {
      return -100;
    }
  }
  t.stop();
  VSA_HIP(hipStreamSynchronize(nullptr));
  c->add_ms += t.ms();
  c->list.n += m;
  c->finished = false;
  c->stats.seen += r->count;
  c->stats.samesequence += totals[VSA_CL_SAME];
  c->stats.mirrordropped += totals[VSA_CL_MIRROR];
  c->stats.rejected += totals[VSA_CL_REJECTED];
  c->stats.edges = c->list.n;
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
  if (c->list.n > 0)
  {
    const int rc = cl_forest(c->rules.numofsequences, c->e1, c->e2, c->list.n,
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
  const uint64_t ne = c->list.n, nseq = c->rules.numofsequences,
                 ncl = c->res.clusters;
  if (ne == 0)
  {
    if (edgestart != nullptr)
    {
      edgestart[0] = 0;
    }
    return records_of(c->list, nullptr, 0, nullptr, nullptr, edges);
  }
  Timer t(nullptr);
  t.start();
  DevBuf order;
  std::vector<uint64_t> hstart;
  rc = cl_group(c->e1, c->e2, ne, c->res.label, nseq, ncl, order, hstart,
                "vsa_cluster_edges");
  if (rc == 0)
  {
    rc = records_of(c->list, order.as<uint32_t>(), ne, palindromic, &t, edges);
  }
  if (rc != 0)
  {
    return rc;
  }
  c->edges_ms += t.ms();
  if (edgestart != nullptr)
  {
    memcpy(edgestart, hstart.data(), (ncl + 1) * 8);
  }
  return 0;
}
