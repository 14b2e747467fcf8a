// The stable compaction of the post-processing stages, for the translation
// units that compact something: select.hip, coverage.hip and, through
// cluster_forest.inc, cluster.hip and matchcluster.hip.  Included inside no
// namespace, after search_host.hpp; everything here lands in an unnamed one.
//
// Three steps over tiles of TC_TILE = VSA_SELECT_TILE items, TC_IPT
// consecutive ones per thread:
//   count  k_tc_count: F::cls(i, payload) names the class of item i, or -1.
//          The classes below NE get one count per tile (NE arrays of nt + 1
//          words, the last one 0), the classes from NE on are only totalled.
//   scan   exclusive_sum() of each array: tile counts -> tile offsets, the
//          total of the class through the pinned page.
//   emit   k_tc_emit: the classes again, a workgroup exclusive sum of the
//          counts of the threads, and F::put(class, rank, i, payload) for
//          every item of a class below NE: rank is its place among the items
//          of its class, in the order of the items.
// tc_count() does the first two, tc_emit() the third; between them the caller
// learns the totals and makes room.  Tile offsets and ranks are 64 bit, the
// counts inside a tile 32 bit.
#define TC_BLOCK 256
#define TC_IPT 4 // items per thread of a tile
#define TC_TILE (TC_BLOCK * TC_IPT)

static_assert(TC_TILE == VSA_SELECT_TILE, "the header names the tile");

namespace
{

template <int NE, int NC, class F>
__global__ void __launch_bounds__(TC_BLOCK)
k_tc_count(F f, uint64_t n, uint64_t *__restrict__ tilecount, uint64_t nt,
           unsigned long long *__restrict__ totals)
{
  const uint64_t tile = vsa_bid();
  if (tile * TC_TILE >= n)
  {
    return;
  }
  __shared__ uint32_t sh[TC_BLOCK / 64];
  const uint64_t k0 = tile * TC_TILE + (uint64_t) threadIdx.x * TC_IPT;
  uint32_t c[NC];
#pragma unroll
  for (int q = 0; q < NC; q++)
  {
    c[q] = 0;
  }
#pragma unroll
  for (int j = 0; j < TC_IPT; j++)
  {
    if (k0 + j < n)
    {
      typename F::Payload p;
      const int cls = f.cls(k0 + j, p);
#pragma unroll
      for (int q = 0; q < NC; q++)
      {
        c[q] += cls == q ? 1u : 0u;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < NC; q++)
  {
    uint32_t total;
    (void) vsa_block_exclusive_scan<0, TC_BLOCK>(c[q], sh, total);
    if (threadIdx.x == 0)
    {
      if (q < NE)
      {
        tilecount[(uint64_t) q * (nt + 1) + tile] = total;
      }
      else if (total != 0)
      {
        atomicAdd(&totals[q], (unsigned long long) total);
      }
    }
  }
}

template <int NE, class F>
__global__ void __launch_bounds__(TC_BLOCK)
k_tc_emit(F f, uint64_t n, const uint64_t *__restrict__ tileoffset,
          uint64_t nt)
{
  const uint64_t tile = vsa_bid();
  if (tile * TC_TILE >= n)
  {
    return;
  }
  __shared__ uint32_t sh[TC_BLOCK / 64];
  const uint64_t k0 = tile * TC_TILE + (uint64_t) threadIdx.x * TC_IPT;
  typename F::Payload p[TC_IPT];
  int cls[TC_IPT];
  uint32_t c[NE];
  uint64_t o[NE];
#pragma unroll
  for (int q = 0; q < NE; q++)
  {
    c[q] = 0;
  }
#pragma unroll
  for (int j = 0; j < TC_IPT; j++)
  {
    cls[j] = k0 + j < n ? f.cls(k0 + j, p[j]) : -1;
#pragma unroll
    for (int q = 0; q < NE; q++)
    {
      c[q] += cls[j] == q ? 1u : 0u;
    }
  }
#pragma unroll
  for (int q = 0; q < NE; q++)
  {
    uint32_t total;
    const uint32_t ex =
        vsa_block_exclusive_scan<0, TC_BLOCK>(c[q], sh, total);
    o[q] = tileoffset[(uint64_t) q * (nt + 1) + tile] + ex;
  }
#pragma unroll
  for (int j = 0; j < TC_IPT; j++)
  {
#pragma unroll
    for (int q = 0; q < NE; q++)
    {
      if (cls[j] == q)
      {
        f.put(q, o[q], k0 + j, p[j]);
        o[q]++;
      }
    }
  }
}

// for the functors whose put() needs nothing of what cls() computed
struct NoPayload
{
};

// out[i] = i (T: uint32_t or uint64_t)
template <typename T>
__global__ void __launch_bounds__(TC_BLOCK)
k_tc_iota(T *__restrict__ out, uint64_t n)
{
  const uint64_t i = vsa_bid() * TC_BLOCK + threadIdx.x;
  if (i < n)
  {
    out[i] = (T) i;
  }
}

// ---- host ---------------------------------------------------------------------

inline uint64_t tilesof(uint64_t n)
{
  return (n + TC_TILE - 1) / TC_TILE;
}

// the grid of a grid-stride kernel over n items
inline dim3 stride_grid(uint64_t n, uint64_t maxblocks)
{
  const uint64_t blocks = (n + TC_BLOCK - 1) / TC_BLOCK;
  return dim3(
      (unsigned int) std::max<uint64_t>(1, std::min(blocks, maxblocks)));
}

// the tile counts of the classes below NE scanned into offsets (NE arrays of
// nt + 1 words), totals[q] = items of class q
template <int NE, int NC, class F>
int tc_count(const F &f, uint64_t n, DevBuf &offsets, uint64_t *totals)
{
  const uint64_t nt = tilesof(n);
  DevBuf counts, tot;
  if (counts.alloc(NE * (nt + 1) * 8) != 0 ||
      offsets.alloc(NE * (nt + 1) * 8) != 0 || tot.alloc(NC * 8) != 0)
  {
    return -100;
  }
  VSA_HIP(hipMemsetAsync(counts.p, 0, NE * (nt + 1) * 8, nullptr));
  VSA_HIP(hipMemsetAsync(tot.p, 0, NC * 8, nullptr));
  k_tc_count<NE, NC, F><<<vsa_grid(nt), TC_BLOCK, 0, nullptr>>>(
      f, n, counts.as<uint64_t>(), nt, tot.as<unsigned long long>());
  VSA_HIP(hipGetLastError());
  for (int q = 0; q < NE; q++)
  {
    if (exclusive_sum(counts.as<uint64_t>() + q * (nt + 1),
                      offsets.as<uint64_t>() + q * (nt + 1), nt, nullptr,
                      &totals[q]) != 0)
    {
      return -100;
    }
  }
  if (NC > NE)
  {
    uint64_t t[NC];
    VSA_HIP(hipMemcpy(t, tot.p, NC * 8, hipMemcpyDeviceToHost));
    for (int q = NE; q < NC; q++)
    {
      totals[q] = t[q];
    }
  }
  return 0;
}

template <int NE, class F>
int tc_emit(const F &f, uint64_t n, DevBuf &offsets)
{
  const uint64_t nt = tilesof(n);
  k_tc_emit<NE, F><<<vsa_grid(nt), TC_BLOCK, 0, nullptr>>>(
      f, n, offsets.as<uint64_t>(), nt);
  VSA_HIP(hipGetLastError());
  return 0;
}

} // namespace
