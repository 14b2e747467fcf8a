// Sequence clustering on the device: vmatch -dbcluster percsmall perclarge
// (Vmatch/vmcluster.c:289-415, kurtz/cluster.c:436-614) on match lists that
// stay in HBM.  The rules -- which record is an edge between which sequences
// -- are cluster_rules.h, the same text the host compiles.
//
//   edges    one lane per record, tiles of VSA_SELECT_TILE records: the two
//            sequences by binary search in markpos, the overlap test.  The
//            accepted records are compacted stably: count per tile, exclusive
//            scan of the tile counts, write in order, behind the edges of the
//            lists added before.  An edge keeps its record and its D/P flag:
//            the caller may free the list.
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

#define CL_BLOCK 256
#define CL_IPT 4
#define CL_TILE (CL_BLOCK * CL_IPT)
#define CL_NONE 0xFFFFFFFFFFFFFFFFull

static_assert(CL_TILE == VSA_SELECT_TILE, "the header names the tile");

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

// exclusive sum of one value per thread of a workgroup; sh: CL_BLOCK / 64
// words of LDS
__device__ __forceinline__ uint32_t cl_block_exscan(uint32_t v, uint32_t *sh,
                                                    uint32_t &total)
{
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1)
  {
    const uint32_t o = __shfl_up(incl, d);
    if (lane >= (uint32_t) d)
    {
      incl += o;
    }
  }
  if (lane == 63)
  {
    sh[wave] = incl;
  }
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < CL_BLOCK / 64; w++)
  {
    const uint32_t x = sh[w];
    before += w < wave ? x : 0;
    all += x;
  }
  __syncthreads();
  total = all;
  return before + incl - v;
}

// ---- stable compaction of the items of class 0 -----------------------------
// F::cls(i, payload) names the class of item i; the items of class 0 are
// written in order through F::put(rank, i, payload), the others only counted
// (totals[class]).

template <class F>
__global__ void __launch_bounds__(CL_BLOCK)
k_cl_count(F f, uint64_t n, uint64_t *__restrict__ tilecount,
           unsigned long long *__restrict__ totals)
{
  const uint64_t tile = vsa_bid();
  if (tile * CL_TILE >= n)
  {
    return;
  }
  __shared__ uint32_t sh[CL_BLOCK / 64];
  const uint64_t k0 = tile * CL_TILE + (uint64_t) threadIdx.x * CL_IPT;
  uint32_t c[VSA_CL_CLASSES];
#pragma unroll
  for (int q = 0; q < VSA_CL_CLASSES; q++)
  {
    c[q] = 0;
  }
#pragma unroll
  for (int j = 0; j < CL_IPT; j++)
  {
    if (k0 + j < n)
    {
      typename F::Payload p;
      const int cls = f.cls(k0 + j, p);
#pragma unroll
      for (int q = 0; q < VSA_CL_CLASSES; q++)
      {
        c[q] += cls == q ? 1u : 0u;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < VSA_CL_CLASSES; q++)
  {
    uint32_t total;
    (void) cl_block_exscan(c[q], sh, total);
    if (threadIdx.x == 0)
    {
      if (q == 0)
      {
        tilecount[tile] = total;
      }
      else if (total != 0)
      {
        atomicAdd(&totals[q], (unsigned long long) total);
      }
    }
  }
}

template <class F>
__global__ void __launch_bounds__(CL_BLOCK)
k_cl_emit(F f, uint64_t n, const uint64_t *__restrict__ tileoffset)
{
  const uint64_t tile = vsa_bid();
  if (tile * CL_TILE >= n)
  {
    return;
  }
  __shared__ uint32_t sh[CL_BLOCK / 64];
  const uint64_t k0 = tile * CL_TILE + (uint64_t) threadIdx.x * CL_IPT;
  typename F::Payload p[CL_IPT];
  int cls[CL_IPT];
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < CL_IPT; j++)
  {
    cls[j] = k0 + j < n ? f.cls(k0 + j, p[j]) : -1;
    c += cls[j] == 0 ? 1u : 0u;
  }
  uint32_t total;
  uint64_t o = tileoffset[tile] + cl_block_exscan(c, sh, total);
#pragma unroll
  for (int j = 0; j < CL_IPT; j++)
  {
    if (cls[j] == 0)
    {
      f.put(o, k0 + j, p[j]);
      o++;
    }
  }
}

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
  __device__ void put(uint64_t rank, uint64_t i, const Payload &p) const
  {
    e1[base + rank] = p.s1;
    e2[base + rank] = p.s2;
    recs[base + rank] = matches[i];
    flags[base + rank] = (uint8_t) (palindromic != 0);
  }
};

struct NoPayload
{
};

// the edges of the forest, in the order of their numbers
struct ForestF
{
  typedef NoPayload Payload;
  const uint8_t *inforest;
  const uint32_t *e1, *e2;
  uint32_t *f1, *f2;

  __device__ int cls(uint64_t i, Payload &) const
  {
    return inforest[i] != 0 ? 0 : 1;
  }
  __device__ void put(uint64_t rank, uint64_t i, const Payload &) const
  {
    f1[rank] = e1[i];
    f2[rank] = e2[i];
  }
};

// ---- the forest --------------------------------------------------------------

__global__ void __launch_bounds__(CL_BLOCK)
k_cl_iota(uint32_t *__restrict__ out, uint64_t n)
{
  const uint64_t i = vsa_bid() * CL_BLOCK + threadIdx.x;
  if (i < n)
  {
    out[i] = (uint32_t) i;
  }
}

// parent[] is flat: parent[x] is the root of x.  Every live edge: dead if its
// ends share a root, else a candidate of both roots.  *crossing counts the
// candidates.
__global__ void __launch_bounds__(CL_BLOCK)
k_cl_pick(const uint32_t *__restrict__ e1, const uint32_t *__restrict__ e2,
          uint64_t nedges, const uint32_t *__restrict__ parent,
          uint8_t *__restrict__ live, unsigned long long *__restrict__ best,
          unsigned long long *__restrict__ crossing)
{
  const uint64_t i = vsa_bid() * CL_BLOCK + threadIdx.x;
  bool cross = false;
  if (i < nedges && live[i] != 0)
  {
    const uint32_t ru = parent[e1[i]], rv = parent[e2[i]];
    if (ru == rv)
    {
      live[i] = 0;
    }
    else
    {
      cross = true;
      atomicMin(&best[ru], (unsigned long long) i);
      atomicMin(&best[rv], (unsigned long long) i);
    }
  }
  const uint64_t b = __ballot(cross);
  if (b != 0 && (threadIdx.x & 63u) == (uint32_t) (__ffsll((unsigned long long) b) - 1))
  {
    atomicAdd(crossing, (unsigned long long) __popcll((unsigned long long) b));
  }
}

// next[x] = the parent of x after this round's hooks; parent[] and best[] are
// only read
__global__ void __launch_bounds__(CL_BLOCK)
k_cl_hook(const uint32_t *__restrict__ e1, const uint32_t *__restrict__ e2,
          const uint32_t *__restrict__ parent,
          const unsigned long long *__restrict__ best, uint64_t nseq,
          uint32_t *__restrict__ next, uint8_t *__restrict__ inforest)
{
  const uint64_t x = vsa_bid() * CL_BLOCK + threadIdx.x;
  if (x >= nseq)
  {
    return;
  }
  uint32_t to = parent[x];
  if (to == (uint32_t) x)
  {
    const unsigned long long b = best[x];
    if (b != CL_NONE)
    {
      const uint32_t ru = parent[e1[b]], rv = parent[e2[b]];
      const uint32_t other = ru == (uint32_t) x ? rv : ru;
      inforest[b] = 1;
      // both roots chose b: the smaller one stays a root
      if (best[other] != b || (uint32_t) x > other)
      {
        to = other;
      }
    }
  }
  next[x] = to;
}

// one jump; in place: whatever a lane reads is an ancestor
__global__ void __launch_bounds__(CL_BLOCK)
k_cl_jump(uint32_t *__restrict__ parent, uint64_t nseq,
          unsigned int *__restrict__ changed)
{
  const uint64_t x = vsa_bid() * CL_BLOCK + threadIdx.x;
  bool ch = false;
  if (x < nseq)
  {
    const uint32_t p = parent[x];
    const uint32_t g = parent[p];
    if (g != p)
    {
      parent[x] = g;
      ch = true;
    }
  }
  if (__ballot(ch) != 0 && (threadIdx.x & 63u) == 0)
  {
    *changed = 1u; // every writer stores the same value
  }
}

// ---- grouping ----------------------------------------------------------------

// position j of the reversed list: edge nedges - 1 - j, keyed by its cluster
__global__ void __launch_bounds__(CL_BLOCK)
k_cl_keys(const uint32_t *__restrict__ e1, const uint32_t *__restrict__ e2,
          uint64_t nedges, const uint32_t *__restrict__ label,
          uint64_t *__restrict__ keys, uint32_t *__restrict__ vals,
          unsigned long long *__restrict__ bad)
{
  const uint64_t j = vsa_bid() * CL_BLOCK + threadIdx.x;
  if (j < nedges)
  {
    const uint64_t i = nedges - 1 - j;
    const uint32_t a = label[e1[i]], b = label[e2[i]];
    if (a != b || a == 0xFFFFFFFFu)
    {
      atomicAdd(bad, 1ull);
    }
    keys[j] = a;
    vals[j] = (uint32_t) i;
  }
}

__global__ void __launch_bounds__(CL_BLOCK)
k_cl_gather(const vsa_match *__restrict__ recs,
            const uint8_t *__restrict__ flags,
            const uint32_t *__restrict__ order, uint64_t n,
            vsa_match *__restrict__ outrecs, uint8_t *__restrict__ outflags)
{
  const uint64_t t = vsa_bid() * CL_BLOCK + threadIdx.x;
  if (t < n)
  {
    const uint32_t i = order[t];
    outrecs[t] = recs[i];
    outflags[t] = flags[i];
  }
}

// start[c] = the first position of the sorted keys that is not below c
__global__ void __launch_bounds__(CL_BLOCK)
k_cl_starts(const uint64_t *__restrict__ keys, uint64_t n, uint64_t nclusters,
            uint64_t *__restrict__ start)
{
  const uint64_t c = vsa_bid() * CL_BLOCK + threadIdx.x;
  if (c <= nclusters)
  {
    uint64_t lo = 0, hi = n;
    while (lo < hi)
    {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (keys[mid] < c)
      {
        lo = mid + 1;
      }
      else
      {
        hi = mid;
      }
    }
    start[c] = lo;
  }
}

// ---- host ----------------------------------------------------------------------

uint64_t tilesof(uint64_t n)
{
  return (n + CL_TILE - 1) / CL_TILE;
}

// tile counts of class 0 scanned into offsets (nt + 1 words); totals[q] =
// items of class q
template <class F>
int cl_count(const F &f, uint64_t n, DevBuf &offsets, uint64_t *totals)
{
  const uint64_t nt = tilesof(n);
  DevBuf counts, tot;
  if (counts.alloc((nt + 1) * 8) != 0 || offsets.alloc((nt + 1) * 8) != 0 ||
      tot.alloc(VSA_CL_CLASSES * 8) != 0)
  {
    return -100;
  }
  VSA_HIP(hipMemsetAsync(counts.p, 0, (nt + 1) * 8, nullptr));
  VSA_HIP(hipMemsetAsync(tot.p, 0, VSA_CL_CLASSES * 8, nullptr));
  k_cl_count<F><<<vsa_grid(nt), CL_BLOCK, 0, nullptr>>>(
      f, n, counts.as<uint64_t>(), tot.as<unsigned long long>());
  VSA_HIP(hipGetLastError());
  if (exclusive_sum(counts.as<uint64_t>(), offsets.as<uint64_t>(), nt, nullptr,
                    &totals[0]) != 0)
  {
    return -100;
  }
  uint64_t t[VSA_CL_CLASSES];
  VSA_HIP(hipMemcpy(t, tot.p, sizeof t, hipMemcpyDeviceToHost));
  for (int q = 1; q < VSA_CL_CLASSES; q++)
  {
    totals[q] = t[q];
  }
  return 0;
}

template <class F>
int cl_emit(const F &f, uint64_t n, DevBuf &offsets)
{
  k_cl_emit<F><<<vsa_grid(tilesof(n)), CL_BLOCK, 0, nullptr>>>(
      f, n, offsets.as<uint64_t>());
  VSA_HIP(hipGetLastError());
  return 0;
}

// room for `need` edges; what is there stays
int reserve(vsa_cluster *c, uint64_t need)
{
  if (need <= c->capacity)
  {
    return 0;
  }
  const uint64_t cap = std::max<uint64_t>(need, 2 * c->capacity);
  DevBuf e1, e2, recs, flags;
  if (e1.alloc(cap * 4) != 0 || e2.alloc(cap * 4) != 0 ||
      recs.alloc(cap * sizeof(vsa_match)) != 0 || flags.alloc(cap) != 0)
  {
    return -100;
  }
  if (c->nedges > 0)
  {
    VSA_HIP(hipMemcpyAsync(e1.p, c->e1, c->nedges * 4, hipMemcpyDeviceToDevice,
                           nullptr));
    VSA_HIP(hipMemcpyAsync(e2.p, c->e2, c->nedges * 4, hipMemcpyDeviceToDevice,
                           nullptr));
    VSA_HIP(hipMemcpyAsync(recs.p, c->recs, c->nedges * sizeof(vsa_match),
                           hipMemcpyDeviceToDevice, nullptr));
    VSA_HIP(hipMemcpyAsync(flags.p, c->flags, c->nedges,
                           hipMemcpyDeviceToDevice, nullptr));
    VSA_HIP(hipStreamSynchronize(nullptr));
  }
  vsa_dev_free(c->e1);
  vsa_dev_free(c->e2);
  vsa_dev_free(c->recs);
  vsa_dev_free(c->flags);
  c->e1 = (uint32_t *) e1.release();
  c->e2 = (uint32_t *) e2.release();
  c->recs = (vsa_match *) recs.release();
  c->flags = (uint8_t *) flags.release();
  c->capacity = cap;
  return 0;
}

// the edges of the minimum spanning forest (weight = edge number) in the
// order of their numbers -> f1 / f2 on the host
int forest(vsa_cluster *c, std::vector<uint32_t> &f1,
           std::vector<uint32_t> &f2, uint64_t *rounds)
{
  const uint64_t nseq = c->rules.numofsequences, ne = c->nedges;
  DevBuf parent, next, live, inforest, best, counters;
  if (parent.alloc(nseq * 4) != 0 || next.alloc(nseq * 4) != 0 ||
      live.alloc(ne) != 0 || inforest.alloc(ne) != 0 ||
      best.alloc(nseq * 8) != 0 || counters.alloc(16) != 0)
  {
    return -100;
  }
  unsigned long long *crossing = counters.as<unsigned long long>();
  unsigned int *changed = (unsigned int *) (crossing + 1);
  k_cl_iota<<<gridfor(nseq), CL_BLOCK, 0, nullptr>>>(parent.as<uint32_t>(),
                                                     nseq);
  VSA_HIP(hipGetLastError());
  VSA_HIP(hipMemsetAsync(live.p, 1, ne, nullptr));
  VSA_HIP(hipMemsetAsync(inforest.p, 0, ne, nullptr));
  *rounds = 0;
  for (;;)
  {
    uint64_t ncross = 0;
    VSA_HIP(hipMemsetAsync(best.p, 0xFF, nseq * 8, nullptr));
    VSA_HIP(hipMemsetAsync(counters.p, 0, 16, nullptr));
    k_cl_pick<<<gridfor(ne), CL_BLOCK, 0, nullptr>>>(
        c->e1, c->e2, ne, parent.as<uint32_t>(), live.as<uint8_t>(),
        best.as<unsigned long long>(), crossing);
    VSA_HIP(hipGetLastError());
    VSA_HIP(hipMemcpy(&ncross, crossing, 8, hipMemcpyDeviceToHost));
    if (ncross == 0)
    {
      break;
    }
    if (*rounds == VSA_CLUSTER_MAXROUNDS)
    {
      VSA_ERROR("vsa_cluster_finish: %lu edges still join different "
                "components after %u rounds", (unsigned long) ncross,
                VSA_CLUSTER_MAXROUNDS);
      return -101;
    }
    (*rounds)++;
    k_cl_hook<<<gridfor(nseq), CL_BLOCK, 0, nullptr>>>(
        c->e1, c->e2, parent.as<uint32_t>(), best.as<unsigned long long>(),
        nseq, next.as<uint32_t>(), inforest.as<uint8_t>());
    VSA_HIP(hipGetLastError());
    std::swap(parent.p, next.p);
    unsigned int ch = 1;
    for (unsigned int jumps = 0; ch != 0; jumps++)
    {
      if (jumps == VSA_CLUSTER_MAXJUMPS)
      {
        VSA_ERROR("vsa_cluster_finish: the components are not flat after %u "
                  "jumps", VSA_CLUSTER_MAXJUMPS);
        return -101;
      }
      VSA_HIP(hipMemsetAsync(changed, 0, 4, nullptr));
      k_cl_jump<<<gridfor(nseq), CL_BLOCK, 0, nullptr>>>(parent.as<uint32_t>(),
                                                         nseq, changed);
      VSA_HIP(hipGetLastError());
      VSA_HIP(hipMemcpy(&ch, changed, 4, hipMemcpyDeviceToHost));
    }
  }
  ForestF ff;
  ff.inforest = inforest.as<uint8_t>();
  ff.e1 = c->e1;
  ff.e2 = c->e2;
  ff.f1 = ff.f2 = nullptr;
  DevBuf offsets, d1, d2;
  uint64_t totals[VSA_CL_CLASSES];
  if (cl_count(ff, ne, offsets, totals) != 0)
  {
    return -100;
  }
  const uint64_t nf = totals[0];
  if (nf >= nseq)
  {
    VSA_ERROR("vsa_cluster_finish: a forest of %lu edges over %lu sequences",
              (unsigned long) nf, (unsigned long) nseq);
    return -101;
  }
  f1.resize(nf);
  f2.resize(nf);
  if (nf > 0)
  {
    if (d1.alloc(nf * 4) != 0 || d2.alloc(nf * 4) != 0)
    {
      return -100;
    }
    ff.f1 = d1.as<uint32_t>();
    ff.f2 = d2.as<uint32_t>();
    if (cl_emit(ff, ne, offsets) != 0)
    {
      return -100;
    }
    VSA_HIP(hipMemcpy(f1.data(), d1.p, nf * 4, hipMemcpyDeviceToHost));
    VSA_HIP(hipMemcpy(f2.data(), d2.p, nf * 4, hipMemcpyDeviceToHost));
  }
  return 0;
}

int enter(const vsa_cluster *c)
{
  if (vsa_set_device(c->device) != 0)
  {
    return -100;
  }
  vsa_dev_set_stream(nullptr);
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
  if (vsa_set_device(device) != 0)
  {
    return -100;
  }
  vsa_dev_set_stream(nullptr);
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
  if (enter(c) != 0)
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
  if (cl_count(ef, r->count, offsets, totals) != 0)
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
    if (cl_emit(ef, r->count, offsets) != 0)
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
  if (enter(c) != 0)
  {
    return -100;
  }
  std::vector<uint32_t> f1, f2;
  uint64_t rounds = 0, changed = 0;
  Timer t(nullptr);
  t.start();
  if (c->nedges > 0)
  {
    const int rc = forest(c, f1, f2, &rounds);
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
  if (enter(c) != 0)
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
  // (the guard owns the list until it is handed over)
  struct Guard
  {
    vsa_result *r;
    ~Guard()
    {
      if (r != nullptr)
      {
        vsa_result_free(r);
      }
    }
  } guard = {res};
  Timer t(nullptr);
  t.start();
  std::vector<uint32_t> hlabel(nseq);
  for (uint64_t s = 0; s < nseq; s++)
  {
    hlabel[s] = c->res.label[s] == VSA_CLUSTER_SINGLET
                    ? 0xFFFFFFFFu
                    : (uint32_t) c->res.label[s];
  }
  DevBuf label, keys, keys2, vals, vals2, bad, starts, oflags;
  if (label.alloc(nseq * 4) != 0 || keys.alloc(ne * 8) != 0 ||
      keys2.alloc(ne * 8) != 0 || vals.alloc(ne * 4) != 0 ||
      vals2.alloc(ne * 4) != 0 || bad.alloc(8) != 0 ||
      starts.alloc((ncl + 1) * 8) != 0 || oflags.alloc(ne) != 0 ||
      vsa_dev_alloc((void **) &res->matches, ne * sizeof(vsa_match)) != 0)
  {
    return -100;
  }
  VSA_HIP(hipMemcpyAsync(label.p, hlabel.data(), nseq * 4,
                         hipMemcpyHostToDevice, nullptr));
  VSA_HIP(hipMemsetAsync(bad.p, 0, 8, nullptr));
  k_cl_keys<<<gridfor(ne), CL_BLOCK, 0, nullptr>>>(
      c->e1, c->e2, ne, label.as<uint32_t>(), keys.as<uint64_t>(),
      vals.as<uint32_t>(), bad.as<unsigned long long>());
  VSA_HIP(hipGetLastError());
  if (sortpairs(keys.as<uint64_t>(), keys2.as<uint64_t>(), vals.as<uint32_t>(),
                vals2.as<uint32_t>(), ne, nullptr) != 0)
  {
    return -100;
  }
  k_cl_gather<<<gridfor(ne), CL_BLOCK, 0, nullptr>>>(
      c->recs, c->flags, vals2.as<uint32_t>(), ne, res->matches,
      oflags.as<uint8_t>());
  VSA_HIP(hipGetLastError());
  k_cl_starts<<<gridfor(ncl + 1), CL_BLOCK, 0, nullptr>>>(
      keys2.as<uint64_t>(), ne, ncl, starts.as<uint64_t>());
  VSA_HIP(hipGetLastError());
  t.stop();
  uint64_t nbad = 0;
  std::vector<uint64_t> hstart(ncl + 1);
  VSA_HIP(hipMemcpy(&nbad, bad.p, 8, hipMemcpyDeviceToHost));
  VSA_HIP(hipMemcpy(hstart.data(), starts.p, (ncl + 1) * 8,
                    hipMemcpyDeviceToHost));
  c->edges_ms += t.ms();
  // the reference's own consistency checks (cluster.c:605-611,
  // vmcluster.c:507-513)
  if (nbad != 0)
  {
    VSA_ERROR("vsa_cluster_edges: the two sequences of %lu edges do not "
              "belong to the same cluster", (unsigned long) nbad);
    return -101;
  }
  if (hstart[0] != 0 || hstart[ncl] != ne)
  {
    VSA_ERROR("number %lu of stored matches differs from number %lu of edges "
              "used for clustering", (unsigned long) hstart[ncl],
              (unsigned long) ne);
    return -101;
  }
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
