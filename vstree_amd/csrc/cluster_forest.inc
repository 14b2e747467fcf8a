// The part of the clustering that does not care what the nodes are, for the
// translation units that cluster something: cluster.hip (the sequences of an
// index, vmatch -dbcluster) and matchcluster.hip (the matches of a list,
// vmatch -pp matchcluster).  Included inside no namespace, after
// resident_list.hpp and the rules of the including file (VSA_CL_CLASSES,
// vsa_clresult); everything here lands in an unnamed one.
//
//   compaction  tile_compact.inc, which this file includes: the functors
//               here and in the including files keep class 0 (NE = 1) and
//               total the VSA_CL_CLASSES - 1 others.
//   forest      cl_forest: the edges (e1[i], e2[i]) over `nodes` nodes that
//               change the state of linkcluster -- the minimum spanning forest
//               with weight = edge number -- by Boruvka rounds, compacted in
//               the order of their numbers, to the host.
//   group       cl_group: every edge keyed by the cluster of its ends; a
//               stable radix sort of the edges in reverse order puts each
//               cluster's edges together in descending number, the order
//               addClusterEdge leaves them in.
// Node and edge numbers are 32 bit: the callers refuse more.
#define CL_NONE 0xFFFFFFFFFFFFFFFFull

#include "tile_compact.inc"

namespace
{

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
  __device__ void put(int, uint64_t rank, uint64_t i, const Payload &) const
  {
    f1[rank] = e1[i];
    f2[rank] = e2[i];
  }
};

// ---- the forest --------------------------------------------------------------

// parent[] is flat: parent[x] is the root of x.  Every live edge: dead if its
// ends share a root, else a candidate of both roots.  *crossing counts the
// candidates.
__global__ void __launch_bounds__(TC_BLOCK)
k_cl_pick(const uint32_t *__restrict__ e1, const uint32_t *__restrict__ e2,
          uint64_t nedges, const uint32_t *__restrict__ parent,
          uint8_t *__restrict__ live, unsigned long long *__restrict__ best,
          unsigned long long *__restrict__ crossing)
{
  const uint64_t i = vsa_bid() * TC_BLOCK + threadIdx.x;
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
  wave_count(cross, crossing);
}

// next[x] = the parent of x after this round's hooks; parent[] and best[] are
// only read
__global__ void __launch_bounds__(TC_BLOCK)
k_cl_hook(const uint32_t *__restrict__ e1, const uint32_t *__restrict__ e2,
          const uint32_t *__restrict__ parent,
          const unsigned long long *__restrict__ best, uint64_t nseq,
          uint32_t *__restrict__ next, uint8_t *__restrict__ inforest)
{
  const uint64_t x = vsa_bid() * TC_BLOCK + threadIdx.x;
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
__global__ void __launch_bounds__(TC_BLOCK)
k_cl_jump(uint32_t *__restrict__ parent, uint64_t nseq,
          unsigned int *__restrict__ changed)
{
  const uint64_t x = vsa_bid() * TC_BLOCK + threadIdx.x;
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
__global__ void __launch_bounds__(TC_BLOCK)
k_cl_keys(const uint32_t *__restrict__ e1, const uint32_t *__restrict__ e2,
          uint64_t nedges, const uint32_t *__restrict__ label,
          uint64_t *__restrict__ keys, uint32_t *__restrict__ vals,
          unsigned long long *__restrict__ bad)
{
  const uint64_t j = vsa_bid() * TC_BLOCK + threadIdx.x;
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

// start[c] = the first position of the sorted keys that is not below c
__global__ void __launch_bounds__(TC_BLOCK)
k_cl_starts(const uint64_t *__restrict__ keys, uint64_t n, uint64_t nclusters,
            uint64_t *__restrict__ start)
{
  const uint64_t c = vsa_bid() * TC_BLOCK + threadIdx.x;
  if (c <= nclusters)
  {
    start[c] = vsa_lowerbound(keys, n, c);
  }
}

// ---- host ----------------------------------------------------------------------

// the edges of the minimum spanning forest (weight = edge number) in the
// order of their numbers -> f1 / f2 on the host
int cl_forest(uint64_t nseq, const uint32_t *e1, const uint32_t *e2,
              uint64_t ne, std::vector<uint32_t> &f1,
              std::vector<uint32_t> &f2, uint64_t *rounds, const char *who)
{
  DevBuf parent, next, live, inforest, best, counters;
  if (parent.alloc(nseq * 4) != 0 || next.alloc(nseq * 4) != 0 ||
      live.alloc(ne) != 0 || inforest.alloc(ne) != 0 ||
      best.alloc(nseq * 8) != 0 || counters.alloc(16) != 0)
  {
    return -100;
  }
  unsigned long long *crossing = counters.as<unsigned long long>();
  unsigned int *changed = (unsigned int *) (crossing + 1);
  k_tc_iota<<<gridfor(nseq), TC_BLOCK, 0, nullptr>>>(parent.as<uint32_t>(),
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
    k_cl_pick<<<gridfor(ne), TC_BLOCK, 0, nullptr>>>(
        e1, e2, ne, parent.as<uint32_t>(), live.as<uint8_t>(),
        best.as<unsigned long long>(), crossing);
    VSA_HIP(hipGetLastError());
    VSA_HIP(hipMemcpy(&ncross, crossing, 8, hipMemcpyDeviceToHost));
    if (ncross == 0)
    {
      break;
    }
    if (*rounds == VSA_CLUSTER_MAXROUNDS)
    {
      VSA_ERROR("%s: %lu edges still join different components after %u "
                "rounds", who, (unsigned long) ncross, VSA_CLUSTER_MAXROUNDS);
      return -101;
    }
    (*rounds)++;
    k_cl_hook<<<gridfor(nseq), TC_BLOCK, 0, nullptr>>>(
        e1, e2, parent.as<uint32_t>(), best.as<unsigned long long>(),
        nseq, next.as<uint32_t>(), inforest.as<uint8_t>());
    VSA_HIP(hipGetLastError());
    std::swap(parent.p, next.p);
    unsigned int ch = 1;
    for (unsigned int jumps = 0; ch != 0; jumps++)
    {
      if (jumps == VSA_CLUSTER_MAXJUMPS)
      {
        VSA_ERROR("%s: the components are not flat after %u jumps", who,
                  VSA_CLUSTER_MAXJUMPS);
        return -101;
      }
      VSA_HIP(hipMemsetAsync(changed, 0, 4, nullptr));
      k_cl_jump<<<gridfor(nseq), TC_BLOCK, 0, nullptr>>>(parent.as<uint32_t>(),
                                                         nseq, changed);
      VSA_HIP(hipGetLastError());
      VSA_HIP(hipMemcpy(&ch, changed, 4, hipMemcpyDeviceToHost));
    }
  }
  ForestF ff;
  ff.inforest = inforest.as<uint8_t>();
  ff.e1 = e1;
  ff.e2 = e2;
  ff.f1 = ff.f2 = nullptr;
  DevBuf offsets, d1, d2;
  uint64_t totals[VSA_CL_CLASSES];
  if (tc_count<1, VSA_CL_CLASSES>(ff, ne, offsets, totals) != 0)
  {
    return -100;
  }
  const uint64_t nf = totals[0];
  if (nf >= nseq)
  {
    VSA_ERROR("%s: a forest of %lu edges over %lu elements", who,
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
    if (tc_emit<1>(ff, ne, offsets) != 0)
    {
      return -100;
    }
    VSA_HIP(hipMemcpy(f1.data(), d1.p, nf * 4, hipMemcpyDeviceToHost));
    VSA_HIP(hipMemcpy(f2.data(), d2.p, nf * 4, hipMemcpyDeviceToHost));
  }
  return 0;
}

// order[t] = the number of the edge at place t when the edges are grouped by
// the cluster label[] gives their ends (VSA_CLUSTER_SINGLET: in no cluster;
// host memory, as vsa_cl_replay leaves it), each group in descending number;
// hstart[c] = the first place of cluster c (ncl + 1 entries).  With the
// reference's own consistency checks (cluster.c:605-611, vmcluster.c:507-513).
int cl_group(const uint32_t *e1, const uint32_t *e2, uint64_t ne,
             const uint64_t *label, uint64_t nnodes, uint64_t ncl,
             DevBuf &order, std::vector<uint64_t> &hstart, const char *who)
{
  std::vector<uint32_t> hlabel(nnodes);
  for (uint64_t x = 0; x < nnodes; x++)
  {
    hlabel[x] = label[x] == VSA_CLUSTER_SINGLET ? 0xFFFFFFFFu
                                                : (uint32_t) label[x];
  }
  DevBuf dlabel, keys, keys2, vals, bad, starts;
  if (dlabel.alloc(nnodes * 4) != 0 || keys.alloc(ne * 8) != 0 ||
      keys2.alloc(ne * 8) != 0 || vals.alloc(ne * 4) != 0 ||
      order.alloc(ne * 4) != 0 || bad.alloc(8) != 0 ||
      starts.alloc((ncl + 1) * 8) != 0)
  {
    return -100;
  }
  VSA_HIP(hipMemcpyAsync(dlabel.p, hlabel.data(), nnodes * 4,
                         hipMemcpyHostToDevice, nullptr));
  VSA_HIP(hipMemsetAsync(bad.p, 0, 8, nullptr));
  k_cl_keys<<<gridfor(ne), TC_BLOCK, 0, nullptr>>>(
      e1, e2, ne, dlabel.as<uint32_t>(), keys.as<uint64_t>(),
      vals.as<uint32_t>(), bad.as<unsigned long long>());
  VSA_HIP(hipGetLastError());
  if (sortpairs(keys.as<uint64_t>(), keys2.as<uint64_t>(), vals.as<uint32_t>(),
                order.as<uint32_t>(), ne, 64, nullptr) != 0)
  {
    return -100;
  }
  k_cl_starts<<<gridfor(ncl + 1), TC_BLOCK, 0, nullptr>>>(
      keys2.as<uint64_t>(), ne, ncl, starts.as<uint64_t>());
  VSA_HIP(hipGetLastError());
  uint64_t nbad = 0;
  hstart.resize(ncl + 1);
  // (the copy of the pageable hlabel[] above is over when these return)
  VSA_HIP(hipMemcpy(&nbad, bad.p, 8, hipMemcpyDeviceToHost));
  VSA_HIP(hipMemcpy(hstart.data(), starts.p, (ncl + 1) * 8,
                    hipMemcpyDeviceToHost));
  if (nbad != 0)
  {
    VSA_ERROR("%s: the two ends of %lu edges do not belong to the same "
              "cluster", who, (unsigned long) nbad);
    return -101;
  }
  if (hstart[0] != 0 || hstart[ncl] != ne)
  {
    VSA_ERROR("number %lu of stored matches differs from number %lu of edges "
              "used for clustering", (unsigned long) hstart[ncl],
              (unsigned long) ne);
    return -101;
  }
  return 0;
}

} // namespace
