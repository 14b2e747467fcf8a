// vmatch -online -complete [remred] [-e K | -h K] on the device: the scan of
// the text without an index (include/vstree_amd_online.h), by the rules of
// online_rules.h, which the host code of online_host.c reads too.
//
// Both device entries go through one driver over a "text view" (the padded
// text of a vsa_index or of a vsa_text).  The queries are taken in chunks
// whose (query, tile) counters fit ON_COUNTERS words (VSA_ONLINE_COUNTERS in
// the environment: fewer; plan() is the arithmetic); per chunk:
//
//   edit distance
//     count    k_online_edist_count: a work-item is (query, tile of T
//              symbols).  A workgroup of ON_BLOCK lanes owns ON_BLOCK
//              consecutive tiles and stages them, with the warm-up symbols
//              to their right, through LDS with coalesced 8-byte loads -- a
//              lane's own reads are T bytes apart, one 128-byte line per
//              lane and load otherwise.  Tile t lies at word t (T / 8 + 1)
//              of the image: the odd stride spreads the lanes over the
//              banks.  Then the workgroup loops over a group of ON_GROUP
//              queries on the staged text; a wavefront works on one query at
//              a time, so the pattern is uniform, and its lanes scan
//              consecutive tiles from right to left, each from a reset
//              column vsa_online_warmup() symbols (rounded up to 8) to the
//              right of its tile.
//     compact  the (query, tile) pairs with a count (tile_compact.inc), in
//              the order of the list: query ascending, tile descending.
//     write    k_online_edist_write: one lane per such pair scans its tile
//              again and writes (position, score) behind the pair's offset.
//     remred   k_online_remred: the lane of the first hit of a run of
//              adjacent positions walks the run with vsa_online_remred_step
//              and marks the positions it flushes; compaction in order.
//     longest  k_online_longest: edistprocessstartpos per start position
//              with maxlength = min(m + k, n - start) (apm_longest_prefix).
//   Hamming distance and exact
//     k_online_window_count / _write: a tile is ON_WTILE start positions, a
//     lane takes one start position per round and compares 8-byte words
//     (vsa_online_word) until k + 1 mismatches or a symbol that bars the
//     window; the same count, compact, write scheme; a workgroup per pair
//     writes in order (ascending for exact, descending for -h).
#include "search_host.hpp"
#include "approx_device.hpp"
#include "online_rules.h"
#include "tile_compact.inc"

#define ON_BLOCK 128 // lanes = tiles of a workgroup of the edit scan
#define ON_GROUP 32  // queries a workgroup loops over on its staged text
#define ON_WBLOCK 256
#define ON_WROUNDS 8
#define ON_WTILE (ON_WBLOCK * ON_WROUNDS) // start positions of a window tile
// (query, tile) counters of one chunk
#define ON_COUNTERS VSA_ONLINE_COUNTERS_DEFAULT
#define ON_MAXGROUPS 65535ull    // the y dimension of a grid

struct vsa_text
{
  int device;
  hipStream_t stream;
  uint64_t n;
  uint32_t numofchars;
  uint8_t *alloc; // the text starts at alloc + VSA_TIS_FRONTPAD
};

namespace
{

// what the driver needs of a vsa_index or a vsa_text
struct TextView
{
  const uint8_t *tis; // [-FRONTPAD, n + BACKPAD), the padding reads as 255
  uint64_t n;
  uint32_t numofchars;
  int device;
  hipStream_t stream;
};

// what every kernel needs of a call
struct OnCall
{
  const uint8_t *tis;
  uint64_t n;
  DevQueries qs;
  uint64_t q0, q1; // the chunk of queries
  uint64_t distvalue;
  int percent, mode;
  uint64_t ntiles;
};

__device__ __forceinline__ void on_query(const OnCall &c, uint64_t q,
                                         const uint8_t *&pattern, uint32_t &m,
                                         uint32_t &k)
{
  if (c.qs.dense)
  {
    pattern = c.qs.symbols + q * c.qs.uniformlen;
    m = c.qs.uniformlen;
  } else
  {
    pattern = c.qs.symbols + c.qs.start[q];
    m = (uint32_t) c.qs.length[q];
  }
  k = c.mode == VSA_ONLINE_EXACT
          ? 0u
          : (uint32_t) vsa_online_threshold(m, c.distvalue, c.percent);
}

// the place of (query, tile) in the list of the pairs: in the order of the
// matches, i.e. tiles descending for the scans that report descending
__device__ __forceinline__ uint64_t on_item(const OnCall &c, uint64_t q,
                                            uint64_t tile)
{
  return (q - c.q0) * c.ntiles +
         (c.mode == VSA_ONLINE_EXACT ? tile : c.ntiles - 1 - tile);
}

__device__ __forceinline__ void on_pair(const OnCall &c, uint64_t item,
                                        uint64_t &q, uint64_t &tile)
{
  const uint64_t t = item % c.ntiles;
  q = c.q0 + item / c.ntiles;
  tile = c.mode == VSA_ONLINE_EXACT ? t : c.ntiles - 1 - t;
}

// ---- edit distance ------------------------------------------------------------

// LDS: (ON_BLOCK * T + warmmax) / 8 words of text and one word of padding
// per tile begun
template <int W>
__global__ void __launch_bounds__(ON_BLOCK)
k_online_edist_count(const OnCall c, uint32_t T, uint32_t warmmax,
                     uint32_t *__restrict__ counts)
{
  extern __shared__ uint64_t on_text[];
  const uint64_t tile0 = (uint64_t) blockIdx.x * ON_BLOCK, a0 = tile0 * T;
  const uint32_t tilewords = T / 8,
                 spanwords = (ON_BLOCK * T + warmmax) / 8;
  for (uint32_t i = threadIdx.x; i < spanwords; i += ON_BLOCK)
  {
    const uint64_t pos = a0 + 8ull * i;
    // (a word that begins inside the text ends inside its padding)
    on_text[i + i / tilewords] = pos < c.n ? vsa_load8(c.tis + pos) : ~0ull;
  }
  __syncthreads();
  const uint32_t lt = threadIdx.x, lo = lt * T, own = lo + T;
  const uint64_t tile = tile0 + lt,
                 g0 = c.q0 + (uint64_t) blockIdx.y * ON_GROUP,
                 g1 = g0 + ON_GROUP < c.q1 ? g0 + ON_GROUP : c.q1;
  if (tile >= c.ntiles)
  {
    return;
  }
  for (uint64_t q = g0; q < g1; q++)
  {
    const uint8_t *pattern;
    uint32_t m, k;
    on_query(c, q, pattern, m, k);
    if (m == 0)
    {
      continue;
    }
    ApmColumn<W> col;
    col.init(pattern, m, true, vsa_online_rawequal(m) != 0);
    // the warm-up: vsa_online_warmup(), DESIGN.md section 4k
    uint32_t rel = own + (((uint32_t) vsa_online_warmup(m, k) + 7u) & ~7u);
    uint32_t tj = (rel - 8) / T, found = 0;
    while (rel > lo)
    {
      rel -= 8;
      const uint32_t wi = rel / 8;
      if (wi < tj * tilewords)
      {
        tj--;
      }
      const uint64_t w8 = on_text[wi + tj];
#pragma unroll
      for (int j = 7; j >= 0; j--)
      {
        const uint8_t s = (uint8_t) (w8 >> (8 * j));
        if (s == VSA_SEPARATOR)
        {
          col.reset();
        } else
        {
          col.template step<0>(s);
          found += (vsa_online_isstart(col.score, k) && rel + j < own) ? 1u
                                                                        : 0u;
        }
      }
    }
    if (found != 0)
    {
      counts[on_item(c, q, tile)] = found;
    }
  }
}

template <int W>
__global__ void __launch_bounds__(VSA_BLOCK)
k_online_edist_write(const OnCall c, uint32_t T,
                     const uint64_t *__restrict__ items,
                     const uint64_t *__restrict__ offsets, uint64_t nitems,
                     uint64_t *__restrict__ hitpos,
                     uint32_t *__restrict__ hitscore,
                     uint32_t *__restrict__ hitq)
{
  const uint64_t r = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (r >= nitems)
  {
    return;
  }
  uint64_t q, tile;
  on_pair(c, items[r], q, tile);
  const uint8_t *pattern;
  uint32_t m, k;
  on_query(c, q, pattern, m, k);
  ApmColumn<W> col;
  col.init(pattern, m, true, vsa_online_rawequal(m) != 0);
  const uint64_t a = tile * T, b = a + T < c.n ? a + T : c.n,
                 warm = vsa_online_warmup(m, k), end = offsets[r + 1];
  int64_t t = (int64_t) (c.n - b > warm ? b + warm : c.n) - 1;
  uint64_t slot = offsets[r];
  while (t >= (int64_t) a)
  {
    // the 8 symbols ending at t (the text has 64 bytes of padding in front)
    const uint64_t w8 = vsa_load8(c.tis + t - 7);
    const int cnt = (t - (int64_t) a + 1 < 8) ? (int) (t - (int64_t) a + 1) : 8;
    for (int j = 0; j < cnt; j++)
    {
      const uint8_t s = (uint8_t) (w8 >> (8 * (7 - j)));
      if (s == VSA_SEPARATOR)
      {
        col.reset();
      } else
      {
        col.template step<0>(s);
        if (vsa_online_isstart(col.score, k) && (uint64_t) (t - j) < b &&
            slot < end)
        {
          hitpos[slot] = (uint64_t) (t - j);
          hitscore[slot] = col.score;
          hitq[slot] = (uint32_t) (q - c.q0);
          slot++;
        }
      }
    }
    t -= cnt;
  }
}

// CHECKMATCHPOSITION over the hits of the chunk: the lane of the first hit
// of a run of adjacent positions of one query walks the run.  A hit that is
// not adjacent in position is not adjacent to the stored position either, so
// the state of a run owes nothing to the run before it.
__global__ void __launch_bounds__(VSA_BLOCK)
k_online_remred(const uint32_t *__restrict__ hitq,
                const uint64_t *__restrict__ hitpos,
                const uint32_t *__restrict__ hitscore, uint64_t nh,
                uint8_t *__restrict__ keep)
{
  const uint64_t i = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (i >= nh ||
      (i > 0 && hitq[i - 1] == hitq[i] && hitpos[i - 1] == hitpos[i] + 1))
  {
    return;
  }
  vsa_online_remred st;
  vsa_online_remred_init(&st);
  uint64_t stored = i, flush;
  for (uint64_t j = i; j < nh; j++)
  {
    if (j > i && !(hitq[j] == hitq[i] && hitpos[j - 1] == hitpos[j] + 1))
    {
      break;
    }
    if (vsa_online_remred_step(&st, hitpos[j], hitscore[j], &flush))
    {
      keep[stored] = 1;
    }
    if (st.relpos == hitpos[j])
    {
      stored = j;
    }
  }
  if (vsa_online_remred_end(&st, &flush))
  {
    keep[stored] = 1;
  }
}

template <int W>
__global__ void __launch_bounds__(VSA_BLOCK)
k_online_longest(const OnCall c, const uint32_t *__restrict__ hitq,
                 const uint64_t *__restrict__ hitpos, uint64_t nh,
                 vsa_match *__restrict__ out)
{
  const uint64_t h = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (h >= nh)
  {
    return;
  }
  const uint64_t q = c.q0 + hitq[h], pos = hitpos[h];
  const uint8_t *pattern;
  uint32_t m, k, bestlen, bestdist;
  on_query(c, q, pattern, m, k);
  apm_longest_prefix<W>(pattern, m, c.tis + pos,
                        (uint32_t) vsa_online_maxlength(m, k, c.n, pos),
                        bestlen, bestdist);
  vsa_match mt;
  mt.length = bestlen;
  mt.dbstart = pos;
  mt.queryseq = q + c.qs.seqoffset;
  mt.querystart = bestdist;
  out[h] = mt;
}

// ---- Hamming distance and exact ---------------------------------------------------

// does the window at pos (pos + m <= n) match?  mm = its unequal symbols
__device__ __forceinline__ bool on_window(const OnCall &c, uint64_t pos,
                                          const uint8_t *pattern, uint32_t m,
                                          uint32_t k, uint32_t &mm)
{
  mm = 0;
  for (uint32_t o = 0; o < m; o += 8)
  {
    // (behind the text and behind the queries there are 64 bytes of padding)
    int barred;
    mm += vsa_online_word(vsa_load8(c.tis + pos + o), vsa_load8(pattern + o),
                          m - o < 8 ? m - o : 8u, c.mode, &barred);
    if (barred || mm > k)
    {
      return false;
    }
  }
  return true;
}

// the start position of a lane in a round: the lanes of a workgroup in the
// order of the matches
__device__ __forceinline__ uint64_t on_wpos(const OnCall &c, uint64_t tile,
                                            uint32_t round)
{
  const uint32_t r = c.mode == VSA_ONLINE_EXACT ? round
                                                : ON_WROUNDS - 1 - round,
                 l = c.mode == VSA_ONLINE_EXACT ? threadIdx.x
                                                : ON_WBLOCK - 1 - threadIdx.x;
  return tile * ON_WTILE + (uint64_t) r * ON_WBLOCK + l;
}

__global__ void __launch_bounds__(ON_WBLOCK)
k_online_window_count(const OnCall c, uint32_t *__restrict__ counts)
{
  __shared__ uint32_t sh[ON_WBLOCK / 64];
  const uint64_t tile = blockIdx.x,
                 g0 = c.q0 + (uint64_t) blockIdx.y * ON_GROUP,
                 g1 = g0 + ON_GROUP < c.q1 ? g0 + ON_GROUP : c.q1;
  for (uint64_t q = g0; q < g1; q++)
  {
    const uint8_t *pattern;
    uint32_t m, k, mm, found = 0, total;
    on_query(c, q, pattern, m, k);
    if (m == 0 || m > c.n)
    {
      continue; // (the same for every lane)
    }
    for (uint32_t round = 0; round < ON_WROUNDS; round++)
    {
      const uint64_t pos = on_wpos(c, tile, round);
      found += (pos <= c.n - m && on_window(c, pos, pattern, m, k, mm)) ? 1u
                                                                         : 0u;
    }
    (void) vsa_block_exclusive_scan<0, ON_WBLOCK>(found, sh, total);
    if (threadIdx.x == 0 && total != 0)
    {
      counts[on_item(c, q, tile)] = total;
    }
  }
}

// one workgroup per (query, tile) pair with matches
__global__ void __launch_bounds__(ON_WBLOCK)
k_online_window_write(const OnCall c, const uint64_t *__restrict__ items,
                      const uint64_t *__restrict__ offsets, uint64_t nitems,
                      vsa_match *__restrict__ out)
{
  __shared__ uint32_t sh[ON_WBLOCK / 64];
  const uint64_t r = vsa_bid();
  if (r >= nitems)
  {
    return;
  }
  uint64_t q, tile, base = offsets[r];
  const uint64_t end = offsets[r + 1];
  on_pair(c, items[r], q, tile);
  const uint8_t *pattern;
  uint32_t m, k;
  on_query(c, q, pattern, m, k);
  for (uint32_t round = 0; round < ON_WROUNDS; round++)
  {
    const uint64_t pos = on_wpos(c, tile, round);
    uint32_t mm = 0, total;
    const bool ok = pos <= c.n - m && on_window(c, pos, pattern, m, k, mm);
    const uint32_t ex =
        vsa_block_exclusive_scan<0, ON_WBLOCK>(ok ? 1u : 0u, sh, total);
    if (ok && base + ex < end)
    {
      vsa_match mt;
      mt.length = m;
      mt.dbstart = pos;
      mt.queryseq = q + c.qs.seqoffset;
      mt.querystart = mm;
      out[base + ex] = mt;
    }
    base += total;
  }
}

// ---- the compactions (tile_compact.inc) ---------------------------------------

// the (query, tile) pairs with a count, and their counts as 64-bit words
struct PairF
{
  typedef NoPayload Payload;
  const uint32_t *counts;
  uint64_t *items, *itemcounts;

  __device__ int cls(uint64_t i, Payload &) const
  {
    return counts[i] != 0 ? 0 : -1;
  }
  __device__ void put(int, uint64_t rank, uint64_t i, const Payload &) const
  {
    items[rank] = i;
    itemcounts[rank] = counts[i];
  }
};

// the start positions remred keeps
struct KeepF
{
  typedef NoPayload Payload;
  const uint8_t *keep;
  const uint32_t *q;
  const uint64_t *pos;
  uint32_t *outq;
  uint64_t *outpos;

  __device__ int cls(uint64_t i, Payload &) const
  {
    return keep[i] != 0 ? 0 : -1;
  }
  __device__ void put(int, uint64_t rank, uint64_t i, const Payload &) const
  {
    outq[rank] = q[i];
    outpos[rank] = pos[i];
  }
};

// ---- host ---------------------------------------------------------------------

// symbols per tile of the edit scan: VSA_ONLINE_TILE, a multiple of 8 from 64
// to the default
uint32_t tilesize()
{
  const char *s = getenv("VSA_ONLINE_TILE");
  uint32_t t = VSA_ONLINE_TILE_DEFAULT;
  if (s != nullptr && *s != '\0')
  {
    const unsigned long v = strtoul(s, nullptr, 10);
    if (v >= 64 && v <= VSA_ONLINE_TILE_DEFAULT)
    {
      t = (uint32_t) v & ~7u;
    }
  }
  return t;
}

// (query, tile) counters of a chunk: VSA_ONLINE_COUNTERS, from 1 to the
// default
uint64_t countersize()
{
  const char *s = getenv("VSA_ONLINE_COUNTERS");
  uint64_t n = ON_COUNTERS;
  if (s != nullptr && *s != '\0')
  {
    const unsigned long long v = strtoull(s, nullptr, 10);
    if (v >= 1 && v <= ON_COUNTERS)
    {
      n = v;
    }
  }
  return n;
}

// how a call cuts its work: the arithmetic of the driver, which
// vsa_online_plan shows to the tests
struct Plan
{
  uint32_t tile;   // symbols (edit scan) or start positions of a tile
  uint64_t ntiles; // 0 for an empty text
  uint64_t step;   // queries of a chunk
  uint64_t chunks; // 0 where nothing is scanned
};

Plan plan(uint64_t n, uint64_t nq, int mode)
{
  Plan p;
  p.tile = mode == VSA_ONLINE_EDIST ? tilesize() : (uint32_t) ON_WTILE;
  p.ntiles = n / p.tile + (n % p.tile != 0 ? 1 : 0);
  p.step = countersize() / std::max<uint64_t>(1, p.ntiles);
  p.step = std::max<uint64_t>(1, p.step);
  p.step = std::min<uint64_t>(p.step, ON_MAXGROUPS * ON_GROUP);
  p.chunks = n > 0 ? nq / p.step + (nq % p.step != 0 ? 1 : 0) : 0;
  return p;
}

struct Chunk
{
  void *matches;
  uint64_t count;
};

struct Totals
{
  uint64_t hits = 0, pairs = 0;
  double scan_ms = 0, first_ms = 0;
};

// the pairs with a count -> items[npairs], offsets[npairs + 1]; *nh = hits
int compact_pairs(const uint32_t *counts, uint64_t nitems, DevBuf &items,
                  DevBuf &offsets, uint64_t *npairs, uint64_t *nh)
{
  PairF f;
  DevBuf tileoffsets, itemcounts;
  uint64_t totals[1];
  f.counts = counts;
  f.items = f.itemcounts = nullptr;
  *npairs = *nh = 0;
  if (tc_count<1, 1>(f, nitems, tileoffsets, totals) != 0)
  {
    return -100;
  }
  if (totals[0] == 0)
  {
    return 0;
  }
  if (items.alloc(totals[0] * 8) != 0 ||
      itemcounts.alloc((totals[0] + 1) * 8) != 0 ||
      offsets.alloc((totals[0] + 1) * 8) != 0)
  {
    return -100;
  }
  f.items = items.as<uint64_t>();
  f.itemcounts = itemcounts.as<uint64_t>();
  VSA_HIP(hipMemsetAsync(f.itemcounts + totals[0], 0, 8, nullptr));
  if (tc_emit<1>(f, nitems, tileoffsets) != 0 ||
      exclusive_sum(f.itemcounts, offsets.as<uint64_t>(), totals[0], nullptr,
                    nh) != 0)
  {
    return -100;
  }
  *npairs = totals[0];
  return 0;
}

template <int W>
int edist_chunk(const OnCall &c, uint32_t T, uint32_t warmmax, bool remred,
                Chunk &out, Totals &tot)
{
  const uint64_t nq = c.q1 - c.q0, nitems = nq * c.ntiles;
  DevBuf counts, items, offsets, hitpos, hitscore, hitq, matches;
  uint64_t npairs, nh;
  Timer t1(nullptr), t2(nullptr);

  if (counts.alloc(nitems * 4) != 0)
  {
    return -100;
  }
  VSA_HIP(hipMemsetAsync(counts.p, 0, nitems * 4, nullptr));
  const uint32_t tilesbegun = ON_BLOCK + warmmax / T + 2;
  const size_t lds = ((size_t) ON_BLOCK * T + warmmax) + 8 * (size_t) tilesbegun;
  const dim3 grid((unsigned int) ((c.ntiles + ON_BLOCK - 1) / ON_BLOCK),
                  (unsigned int) ((nq + ON_GROUP - 1) / ON_GROUP));
  t1.start();
  k_online_edist_count<W><<<grid, ON_BLOCK, lds, nullptr>>>(
      c, T, warmmax, counts.as<uint32_t>());
  t1.stop();
  VSA_HIP(hipGetLastError());
  if (compact_pairs(counts.as<uint32_t>(), nitems, items, offsets, &npairs,
                    &nh) != 0)
  {
    return -100;
  }
  tot.first_ms += t1.ms();
  tot.scan_ms += t1.ms();
  if (nh == 0)
  {
    return 0;
  }
  if (nh >= 0xFFFFFFFFull)
  {
    VSA_ERROR("%lu start positions of %lu queries are not covered by the GPU "
              "engine", (unsigned long) nh, (unsigned long) nq);
    return VSA_NOT_COVERED;
  }
  counts.free();
  if (hitpos.alloc(nh * 8) != 0 || hitscore.alloc(nh * 4) != 0 ||
      hitq.alloc(nh * 4) != 0)
  {
    return -100;
  }
  t2.start();
  k_online_edist_write<W><<<gridfor(npairs), VSA_BLOCK, 0, nullptr>>>(
      c, T, items.as<uint64_t>(), offsets.as<uint64_t>(), npairs,
      hitpos.as<uint64_t>(), hitscore.as<uint32_t>(), hitq.as<uint32_t>());
  t2.stop();
  VSA_HIP(hipGetLastError());
  tot.hits += nh;
  tot.pairs += npairs;
  uint64_t nstarts = nh;
  DevBuf keptq, keptpos;
  const uint32_t *sq = hitq.as<uint32_t>();
  const uint64_t *spos = hitpos.as<uint64_t>();
  if (remred)
  {
    DevBuf keep, tileoffsets;
    KeepF f;
    uint64_t totals[1];
    if (keep.alloc(nh) != 0)
    {
      return -100;
    }
    VSA_HIP(hipMemsetAsync(keep.p, 0, nh, nullptr));
    k_online_remred<<<gridfor(nh), VSA_BLOCK, 0, nullptr>>>(
        hitq.as<uint32_t>(), hitpos.as<uint64_t>(), hitscore.as<uint32_t>(),
        nh, keep.as<uint8_t>());
    VSA_HIP(hipGetLastError());
    f.keep = keep.as<uint8_t>();
    f.q = sq;
    f.pos = spos;
    f.outq = nullptr;
    f.outpos = nullptr;
    if (tc_count<1, 1>(f, nh, tileoffsets, totals) != 0 ||
        keptq.alloc(totals[0] * 4) != 0 || keptpos.alloc(totals[0] * 8) != 0)
    {
      return -100;
    }
    f.outq = keptq.as<uint32_t>();
    f.outpos = keptpos.as<uint64_t>();
    if (tc_emit<1>(f, nh, tileoffsets) != 0)
    {
      return -100;
    }
    VSA_HIP(hipStreamSynchronize(nullptr)); // (keep is freed here)
    nstarts = totals[0];
    sq = f.outq;
    spos = f.outpos;
  }
  if (matches.alloc(nstarts * sizeof(vsa_match)) != 0)
  {
    return -100;
  }
  k_online_longest<W><<<gridfor(nstarts), VSA_BLOCK, 0, nullptr>>>(
      c, sq, spos, nstarts, matches.as<vsa_match>());
  VSA_HIP(hipGetLastError());
  VSA_HIP(hipStreamSynchronize(nullptr));
  tot.scan_ms += t2.ms();
  out.count = nstarts;
  out.matches = matches.release();
  return 0;
}

int window_chunk(const OnCall &c, Chunk &out, Totals &tot)
{
  const uint64_t nq = c.q1 - c.q0, nitems = nq * c.ntiles;
  DevBuf counts, items, offsets, matches;
  uint64_t npairs, nh;
  Timer t1(nullptr), t2(nullptr);

  if (counts.alloc(nitems * 4) != 0)
  {
    return -100;
  }
  VSA_HIP(hipMemsetAsync(counts.p, 0, nitems * 4, nullptr));
  const dim3 grid((unsigned int) c.ntiles,
                  (unsigned int) ((nq + ON_GROUP - 1) / ON_GROUP));
  t1.start();
  k_online_window_count<<<grid, ON_WBLOCK, 0, nullptr>>>(
      c, counts.as<uint32_t>());
  t1.stop();
  VSA_HIP(hipGetLastError());
  if (compact_pairs(counts.as<uint32_t>(), nitems, items, offsets, &npairs,
                    &nh) != 0)
  {
    return -100;
  }
  tot.first_ms += t1.ms();
  tot.scan_ms += t1.ms();
  if (nh == 0)
  {
    return 0;
  }
  if (matches.alloc(nh * sizeof(vsa_match)) != 0)
  {
    return -100;
  }
  t2.start();
  k_online_window_write<<<vsa_grid(npairs), ON_WBLOCK, 0, nullptr>>>(
      c, items.as<uint64_t>(), offsets.as<uint64_t>(), npairs,
      matches.as<vsa_match>());
  t2.stop();
  VSA_HIP(hipGetLastError());
  VSA_HIP(hipStreamSynchronize(nullptr));
  tot.scan_ms += t2.ms();
  tot.hits += nh;
  tot.pairs += npairs;
  out.count = nh;
  out.matches = matches.release();
  return 0;
}

int online_run(const TextView &tv, const vsa_queries *queries, int mode,
               uint64_t distvalue, int percent, int removeredundant,
               vsa_result **result)
{
  const char *who = "vsa_findcompletematches_online";
  *result = nullptr;
  if (queries->device != tv.device)
  {
    VSA_ERROR("queries live on device %d, the text on device %d",
              queries->device, tv.device);
    return -1;
  }
  if (mode < VSA_ONLINE_EXACT || mode > VSA_ONLINE_HAMMING || percent < 0 ||
      percent > 2)
  {
    VSA_ERROR("%s: mode %d, percent %d: expected mode 0 (exact), 1 (-e) or 2 "
              "(-h) and percent 0, 1 or 2", who, mode, percent);
    return -2;
  }
  if (removeredundant && mode != VSA_ONLINE_EDIST)
  {
    // Vmatch/parsevm.c:1448
    VSA_ERROR("argument \"remred\" of option -complete requires options -e "
              "or -h");
    return -2;
  }
  if (percent == 2)
  {
    VSA_ERROR("%s: -online with Kb (best of) is not covered by the GPU "
              "engine", who);
    return VSA_NOT_COVERED;
  }
  const uint64_t nq = queries->nq;
  if (nq >= (1ull << 31) || queries->maxlength >= 0xFFFFFFF0ull)
  {
    VSA_ERROR("%s: %lu queries of up to %lu symbols are not covered by the "
              "GPU engine", who, (unsigned long) nq,
              (unsigned long) queries->maxlength);
    return VSA_NOT_COVERED;
  }
  if (mode == VSA_ONLINE_EDIST && nq > 0)
  {
    if (tv.numofchars != 4)
    {
      VSA_ERROR("%s: -e on alphabets of %lu symbols is not covered by the "
                "GPU engine", who, (unsigned long) tv.numofchars);
      return VSA_NOT_COVERED;
    }
    if (queries->maxlength > 64 * VSA_APM_MAXWORDS)
    {
      VSA_ERROR("%s: -e with a query of %lu symbols (more than %d) is not "
                "covered by the GPU engine", who,
                (unsigned long) queries->maxlength, 64 * VSA_APM_MAXWORDS);
      return VSA_NOT_COVERED;
    }
    if (percent ? distvalue >= 100 : distvalue >= queries->minlength)
    {
      VSA_ERROR("%s: a threshold >= the length of a query (every position "
                "matches) is not covered by the GPU engine", who);
      return VSA_NOT_COVERED;
    }
  }
  if (enter(tv.device) != 0)
  {
    return -100;
  }
  // what is queued on the stream of the handle (uploads) is waited for; the
  // scan itself runs on the default stream, as the compaction does
  if (queries->rows != nullptr &&
      vsa_queries_bytes(queries, tv.stream) != 0)
  {
    return -100;
  }
  VSA_HIP(hipStreamSynchronize(tv.stream));
  ResultGuard guard{newresult(tv.device)};
  vsa_result *res = guard.r;
  Timer tall(nullptr);
  Totals tot;
  std::vector<Chunk> chunks;
  auto drop = [&]() {
    for (const Chunk &ch : chunks)
    {
      vsa_dev_free(ch.matches);
    }
  };
  tall.start();
  int rc = 0;
  if (nq > 0 && tv.n > 0)
  {
    OnCall c;
    c.tis = tv.tis;
    c.n = tv.n;
    c.qs = devqueries(queries);
    c.distvalue = distvalue;
    c.percent = percent;
    c.mode = mode;
    const Plan pl = plan(tv.n, nq, mode);
    const uint32_t T = pl.tile; // (of the edit scan only)
    c.ntiles = pl.ntiles;
    const uint64_t maxm = queries->maxlength,
                   maxk = vsa_online_threshold(maxm, distvalue, percent);
    const uint32_t warmmax =
        ((uint32_t) vsa_online_warmup(maxm, maxk < maxm ? maxk : maxm) + 7u) &
        ~7u;
    const uint64_t step = pl.step;
    for (uint64_t q0 = 0; q0 < nq && rc == 0; q0 += step)
    {
      Chunk ch = {nullptr, 0};
      c.q0 = q0;
      c.q1 = std::min(nq, q0 + step);
      if (mode != VSA_ONLINE_EDIST)
      {
        rc = window_chunk(c, ch, tot);
      } else if (maxm <= 64)
      {
        rc = edist_chunk<1>(c, T, warmmax, removeredundant != 0, ch, tot);
      } else if (maxm <= 128)
      {
        rc = edist_chunk<2>(c, T, warmmax, removeredundant != 0, ch, tot);
      } else if (maxm <= 256)
      {
        rc = edist_chunk<4>(c, T, warmmax, removeredundant != 0, ch, tot);
      } else
      {
        rc = edist_chunk<8>(c, T, warmmax, removeredundant != 0, ch, tot);
      }
      if (ch.matches != nullptr)
      {
        chunks.push_back(ch);
      }
    }
  }
  if (rc != 0)
  {
    drop();
    (void) hipStreamSynchronize(nullptr);
    return rc;
  }
  uint64_t n = 0;
  for (const Chunk &ch : chunks)
  {
    n += ch.count;
  }
  DevBuf all;
  if (chunks.size() == 1)
  {
    all.p = chunks[0].matches;
    chunks.clear();
  } else if (n > 0)
  {
    if (all.alloc(n * sizeof(vsa_match)) != 0)
    {
      drop();
      return -100;
    }
    uint64_t at = 0;
    for (const Chunk &ch : chunks)
    {
      if (hipMemcpyAsync(all.as<vsa_match>() + at, ch.matches,
                         ch.count * sizeof(vsa_match),
                         hipMemcpyDeviceToDevice, nullptr) != hipSuccess)
      {
        VSA_ERROR("%s: copy of a chunk of matches failed", who);
        drop();
        return -100;
      }
      at += ch.count;
    }
    if (hipStreamSynchronize(nullptr) != hipSuccess)
    {
      drop();
      return -100;
    }
    drop();
    chunks.clear();
  }
  tall.stop();
  VSA_HIP(hipStreamSynchronize(nullptr));
  res->count = res->stats.count = n;
  res->matches = (vsa_match *) all.release();
  res->stats.candidates = tot.hits;
  res->stats.searches = tot.pairs;
  res->stats.search_kernel_ms = tot.scan_ms;
  res->stats.first_kernel_ms = tot.first_ms;
  res->stats.total_device_ms = tall.ms();
  if (sumlengths(res->matches, n, nullptr, &res->stats.sumlength) != 0)
  {
    return -100;
  }
  guard.r = nullptr;
  *result = res;
  return 0;
}

// a text of n symbols with its padding; the symbols are the caller's to fill
int text_alloc(uint64_t n, uint32_t numofchars, int device, vsa_text **out)
{
  *out = nullptr;
  if (numofchars == 0 || numofchars > 253)
  {
    VSA_ERROR("numofchars=%u: not an alphabet", numofchars);
    return -2;
  }
  if (vsa_set_device(device) != 0)
  {
    return -100;
  }
  vsa_text *t = new vsa_text;
  t->device = device;
  t->stream = nullptr;
  t->n = n;
  t->numofchars = numofchars;
  t->alloc = nullptr;
  *out = t;
  VSA_HIP(hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking));
  VSA_HIP(vsa_hip_malloc((void **) &t->alloc,
                         VSA_TIS_FRONTPAD + n + VSA_TIS_BACKPAD));
  VSA_HIP(hipMemsetAsync(t->alloc, 0xFF, VSA_TIS_FRONTPAD, t->stream));
  VSA_HIP(hipMemsetAsync(t->alloc + VSA_TIS_FRONTPAD + n, 0xFF,
                         VSA_TIS_BACKPAD, t->stream));
  return 0;
}

int text_fill(const void *src, uint64_t n, uint32_t numofchars, int device,
              hipMemcpyKind kind, vsa_text **text)
{
  if (text == nullptr || (src == nullptr && n > 0))
  {
    VSA_ERROR("vsa_text: NULL argument");
    return -1;
  }
  int rc = text_alloc(n, numofchars, device, text);
  if (rc == 0 && n > 0 &&
      hipMemcpyAsync((*text)->alloc + VSA_TIS_FRONTPAD, src, n, kind,
                     (*text)->stream) != hipSuccess)
  {
    VSA_ERROR("vsa_text: copy of the text failed");
    rc = -100;
  }
  if (rc == 0 && hipStreamSynchronize((*text)->stream) != hipSuccess)
  {
    VSA_ERROR("vsa_text: copy of the text failed");
    rc = -100;
  }
  if (rc != 0)
  {
    vsa_text_close(*text);
    *text = nullptr;
  }
  return rc;
}

} // namespace

extern "C" int vsa_online_plan(uint64_t totallength, uint64_t numofqueries,
                               int mode, uint32_t *tile, uint64_t *ntiles,
                               uint64_t *queries_per_chunk,
                               uint64_t *numofchunks)
{
  if (tile == nullptr || ntiles == nullptr || queries_per_chunk == nullptr ||
      numofchunks == nullptr)
  {
    VSA_ERROR("vsa_online_plan: NULL argument");
    return -1;
  }
  if (mode < VSA_ONLINE_EXACT || mode > VSA_ONLINE_HAMMING)
  {
    VSA_ERROR("vsa_online_plan: mode %d: expected mode 0 (exact), 1 (-e) or 2 "
              "(-h)", mode);
    return -2;
  }
  const Plan p = plan(totallength, numofqueries, mode);
  *tile = p.tile;
  *ntiles = p.ntiles;
  *queries_per_chunk = p.step;
  *numofchunks = p.chunks;
  return 0;
}

extern "C" int vsa_text_from_host(const uint8_t *tis, uint64_t totallength,
                                  uint32_t numofchars, int device,
                                  vsa_text **text)
{
  return text_fill(tis, totallength, numofchars, device,
                   hipMemcpyHostToDevice, text);
}

extern "C" int vsa_text_from_device(const void *device_tis,
                                    uint64_t totallength, uint32_t numofchars,
                                    int device, vsa_text **text)
{
  return text_fill(device_tis, totallength, numofchars, device,
                   hipMemcpyDeviceToDevice, text);
}

extern "C" void vsa_text_close(vsa_text *t)
{
  if (t == nullptr)
  {
    return;
  }
  (void) hipSetDevice(t->device);
  (void) hipFree(t->alloc);
  if (t->stream != nullptr)
  {
    vsa_dev_forget_stream(t->stream);
    (void) hipStreamDestroy(t->stream);
  }
  delete t;
}

extern "C" int vsa_findcompletematches_online(const vsa_index *index,
                                              const vsa_queries *queries,
                                              int mode, uint64_t distvalue,
                                              int percent,
                                              int removeredundant,
                                              vsa_result **result)
{
  if (index == nullptr || queries == nullptr || result == nullptr)
  {
    VSA_ERROR("vsa_findcompletematches_online: NULL argument");
    return -1;
  }
  *result = nullptr;
  if (index->bck == nullptr)
  {
    // (an index without bck may have been made without its text)
    VSA_ERROR("table bck is not loaded: the text is only known to be there "
              "with it");
    return -3;
  }
  const TextView tv = {index->tis_alloc + VSA_TIS_FRONTPAD, index->n,
                       index->numofchars, index->device, index->stream};
  return online_run(tv, queries, mode, distvalue, percent, removeredundant,
                    result);
}

extern "C" int vsa_text_findcompletematches_online(
    const vsa_text *text, const vsa_queries *queries, int mode,
    uint64_t distvalue, int percent, int removeredundant, vsa_result **result)
{
  if (text == nullptr || queries == nullptr || result == nullptr)
  {
    VSA_ERROR("vsa_text_findcompletematches_online: NULL argument");
    return -1;
  }
  *result = nullptr;
  const TextView tv = {text->alloc + VSA_TIS_FRONTPAD, text->n,
                       text->numofchars, text->device, text->stream};
  return online_run(tv, queries, mode, distvalue, percent, removeredundant,
                    result);
}
