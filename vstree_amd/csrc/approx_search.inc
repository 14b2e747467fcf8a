// Approximate complete matches on the index, vmatch -complete -e K | -h K
// (BASELINE.json configs[4]); included by esa_search.hip inside its
// anonymous namespace.
//
// Reference: findapproxcompletematchesindex (Vmengine/approxcompl.c:138-199)
// -> splitesaapm / realsplitesaapm (Vmengine/splitesaapm.c:369-558):
//   the pattern is cut into splitsize pieces (getoptsplit :317-353); every
//   index hit of a piece gives the text region an occurrence of the whole
//   pattern around it can cover (storeapmposition :268-302); overlapping and
//   adjacent regions are merged (kurtz/regionsmerger.c:318-357); merged
//   regions are visited in ascending order and scanned from right to left
//   (verifyedist*match :44-196, verifyhammingmatch :198-250); every start
//   position of an occurrence with <= K errors is reported, for edit distance
//   with the best-distance, then longest prefix of the text behind it
//   (edistprocessstartpos approxcompl.c:14-66, longestmatch.c:18-153).
//
// Covered here: piece threshold K/splitsize == 0 with at least two pieces
// (the pigeonhole case: read lengths like m=150,K=2 or m=100,K=2), pieces not
// shorter than prefixlength, 4-letter alphabets, m <= 512 (text positions in
// the width of the index tables: texts of 2^32 symbols and more too).  The
// other configurations -- a piece threshold > 0, patterns that are not cut,
// Hamming distance with a wildcard in a read -- answer VSA_NOT_COVERED here
// and are taken by approx_tree.inc (the caller, vsa_findapproxcompletematches,
// tries that next).
//
//   A1  k_complete_search on all pieces of all queries (the K1 kernel)
//   A2  k_apm_regions      one work-item per piece hit: (query, lo) key, hi
//       radix sort by key; exclusive max-scan = running right end;
//       k_apm_flags / k_apm_writeregions: merged regions in (query, lo) order
//   A3  k_apm_verify_edist one work-item per region: Myers columns in 64-bit
//       words, run twice (count, then write start positions, descending)
//       k_apm_longest      one work-item per start position
//   A3h k_apm_verify_hamming  one work-item per region (count, then write)
#include "approx_device.hpp"
#include <cmath>

// Vmengine/splitesaapm.c:317-353, in the same double arithmetic
static uint64_t apm_getoptsplit(bool doedist, uint64_t spliterrorbound,
                                uint64_t numofchars, uint64_t textlen,
                                uint64_t patternlength, uint64_t threshold)
{
  uint64_t optsplit;

  if (threshold * spliterrorbound >= patternlength)
  {
    optsplit = threshold;
  } else
  {
    const double logtextlen = log((double) textlen),
                 lognumofchars = log((double) numofchars);
    if (doedist)
    {
      optsplit = (uint64_t) ((patternlength + threshold) /
                             (logtextlen / lognumofchars));
    } else
    {
      optsplit = (uint64_t) (patternlength / (logtextlen / lognumofchars));
    }
    if (optsplit > threshold + 1)
    {
      optsplit = threshold + 1;
    }
  }
  while (patternlength > 32 * optsplit) // DPWORDSIZE4
  {
    optsplit++;
  }
  return optsplit;
}

__device__ __forceinline__ void apm_query(const DevQueries &qs, uint64_t q,
                                          const uint8_t *&pattern,
                                          uint32_t &m)
{
  if (qs.dense)
  {
    pattern = qs.symbols + q * qs.uniformlen;
    m = qs.uniformlen;
  } else
  {
    pattern = qs.symbols + qs.start[q];
    m = (uint32_t) qs.length[q];
  }
}

// pieces of query q: offsets 0, splitlen, 2*splitlen, ... while a whole
// piece fits (realsplitesaapm, splitesaapm.c:378-379)
__global__ void __launch_bounds__(VSA_BLOCK)
k_apm_pieces(const DevQueries qs, uint64_t nq,
             const uint32_t *__restrict__ qsplitlen,
             const uint64_t *__restrict__ qpiecebase,
             uint64_t *__restrict__ pstart, uint64_t *__restrict__ plen,
             uint32_t *__restrict__ pquery, uint32_t *__restrict__ ppoffset)
{
  const uint64_t q = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (q >= nq)
  {
    return;
  }
  const uint8_t *pattern;
  uint32_t m;
  apm_query(qs, q, pattern, m);
  const uint32_t sl = qsplitlen[q];
  uint64_t p = qpiecebase[q];
  for (uint32_t off = 0; off + sl <= m; off += sl, p++)
  {
    pstart[p] = (uint64_t) (pattern - qs.symbols) + off;
    plen[p] = sl;
    pquery[p] = (uint32_t) q;
    ppoffset[p] = off;
  }
}

// does any query hold a special symbol?  (Hamming distance compares raw
// bytes in the reference, esahamming.c:66: such batches are not covered)
__global__ void __launch_bounds__(VSA_BLOCK)
k_apm_anyspecial(const DevQueries qs, uint64_t nq,
                 uint32_t *__restrict__ flag)
{
  const uint64_t q = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (q >= nq)
  {
    return;
  }
  const uint8_t *pattern;
  uint32_t m;
  apm_query(qs, q, pattern, m);
  bool special = false;
  for (uint32_t i = 0; i < m; i++)
  {
    special |= VSA_ISSPECIAL(pattern[i]);
  }
  if (special)
  {
    atomicOr(flag, 1u);
  }
}

// storeapmposition, splitesaapm.c:268-302, for every piece hit.  One
// workgroup takes VSA_BLOCK consecutive pieces: their hits are one contiguous
// stretch of the list, filled side by side; which piece a hit belongs to is a
// binary search among the workgroup's own 256 offsets in LDS (not among all
// 50 M of them in memory, 26 dependent loads per hit).
// POS: the type a text position is kept in (32 bits, 64 for texts of 2^32
// symbols and more); pbits: the bits of a sort key (query << pbits | position)
// that hold the position
template <typename IDX, typename POS>
__global__ void __launch_bounds__(VSA_BLOCK)
k_apm_regions(const DevIndex<IDX> ix, const DevQueries qs, uint64_t npieces,
              const uint64_t *__restrict__ left,
              const uint64_t *__restrict__ offsets, uint64_t total,
              const uint32_t *__restrict__ pquery,
              const uint32_t *__restrict__ ppoffset,
              const uint32_t *__restrict__ qk, bool doedist, uint32_t pbits,
              uint64_t *__restrict__ keys, POS *__restrict__ his)
{
  __shared__ uint64_t rel[VSA_BLOCK + 1], pleft[VSA_BLOCK];
  __shared__ uint32_t pq[VSA_BLOCK], ppo[VSA_BLOCK];
  const uint64_t p0 = vsa_bid() * VSA_BLOCK;
  const uint32_t t = threadIdx.x,
                 here = (uint32_t) (npieces - p0 < VSA_BLOCK ? npieces - p0
                                                             : VSA_BLOCK);
  const uint64_t b0 = offsets[p0];
  if (t < here)
  {
    rel[t] = offsets[p0 + t] - b0;
    pleft[t] = left[p0 + t];
    pq[t] = pquery[p0 + t];
    ppo[t] = ppoffset[p0 + t];
  }
  if (t == 0)
  {
    rel[here] = offsets[p0 + here] - b0; // offsets has npieces + 1 entries
  }
  __syncthreads();
  const uint64_t blocktotal = rel[here];
  for (uint64_t i = t; i < blocktotal; i += VSA_BLOCK)
  {
    // the piece whose stretch holds hit i: last k with rel[k] <= i
    uint32_t lo = 0, hi = here;
    while (hi - lo > 1)
    {
      const uint32_t mid = (lo + hi) >> 1;
      if (rel[mid] <= i)
      {
        lo = mid;
      } else
      {
        hi = mid;
      }
    }
    const uint64_t s = (uint64_t) ix.suf[pleft[lo] + (i - rel[lo])];
    const uint32_t q = pq[lo], poffset = ppo[lo], k = qk[q];
    const uint8_t *pattern;
    uint32_t m;
    apm_query(qs, q, pattern, m);
    const uint64_t start = doedist ? (uint64_t) k + poffset : poffset;
    const uint64_t end = doedist ? (uint64_t) m + k - poffset
                                 : (uint64_t) m - poffset;
    const uint64_t rlo = (start > s) ? 0 : s - start;
    const uint64_t rhi = (end + s - 1 < ix.n) ? end + s - 1 : ix.n - 1;
    keys[b0 + i] = ((uint64_t) q << pbits) | rlo;
    his[b0 + i] = (POS) rhi;
  }
  (void) total;
}

// The region keys come out of k_apm_regions grouped by query already (piece
// after piece); what is left to do is the order inside a query, a handful of
// entries: one work-item per query sorts them where they are (stable, like
// the radix sort it stands in for).  A query with more than VSA_APM_SEGMAX
// hits (repeats) raises *big: the batch then takes the radix sort.
#define VSA_APM_SEGMAX 64u

template <typename POS>
__global__ void __launch_bounds__(VSA_BLOCK)
k_apm_sortsegments(const uint64_t *__restrict__ piecebase,
                   const uint64_t *__restrict__ offsets, uint64_t nq,
                   uint64_t *__restrict__ keys, POS *__restrict__ his,
                   unsigned int *__restrict__ big)
{
  const uint64_t q = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (q >= nq)
  {
    return;
  }
  const uint64_t b = offsets[piecebase[q]], e = offsets[piecebase[q + 1]];
  if (e - b <= 1)
  {
    return;
  }
  if (e - b > VSA_APM_SEGMAX)
  {
    atomicOr(big, 1u);
    return;
  }
  for (uint64_t a = b + 1; a < e; a++)
  {
    const uint64_t k = keys[a];
    const POS h = his[a];
    uint64_t c = a;
    while (c > b && keys[c - 1] > k)
    {
      keys[c] = keys[c - 1];
      his[c] = his[c - 1];
      c--;
    }
    keys[c] = k;
    his[c] = h;
  }
}

template <typename POS>
__global__ void __launch_bounds__(VSA_BLOCK)
k_apm_rightends(const uint64_t *__restrict__ keys,
                const POS *__restrict__ his, uint64_t total, uint32_t pbits,
                uint64_t *__restrict__ ends)
{
  const uint64_t t = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (t < total)
  {
    ends[t] = ((keys[t] >> pbits) << pbits) | his[t];
  }
}

// a region starts a new merged region unless it overlaps or touches what is
// to the left of it in the same query (regionsmerger.c:196-213: uint1 + 1
// >= uint0); prev = running maximum of (query, right end) over the hits in
// front of this one
__global__ void __launch_bounds__(VSA_BLOCK)
k_apm_flags(const uint64_t *__restrict__ keys,
            const uint64_t *__restrict__ prev, uint64_t total, uint32_t pbits,
            uint32_t *__restrict__ flags)
{
  const uint64_t t = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (t < total)
  {
    const uint64_t key = keys[t], pr = prev[t];
    const uint64_t mask = (1ull << pbits) - 1;
    const bool fresh = t == 0 || (pr >> pbits) != (key >> pbits) ||
                       (key & mask) > (pr & mask) + 1;
    flags[t] = fresh ? 1u : 0u;
  }
}

template <typename POS>
__global__ void __launch_bounds__(VSA_BLOCK)
k_apm_writeregions(const uint64_t *__restrict__ keys,
                   const uint64_t *__restrict__ ends,
                   const uint64_t *__restrict__ prev,
                   const uint32_t *__restrict__ flags,
                   const uint32_t *__restrict__ rank, uint64_t total,
                   uint32_t pbits, uint32_t *__restrict__ rq,
                   POS *__restrict__ rlo, POS *__restrict__ rhi,
                   uint32_t *__restrict__ rfirst)
{
  const uint64_t t = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (t >= total)
  {
    return;
  }
  const uint32_t r = rank[t] - 1; // rank = inclusive scan of flags
  const uint64_t mask = (1ull << pbits) - 1;
  if (flags[t] != 0)
  {
    rq[r] = (uint32_t) (keys[t] >> pbits);
    rlo[r] = (POS) (keys[t] & mask);
    rfirst[r] = (uint32_t) t;
  }
  if (t + 1 == total)
  {
    rfirst[r + 1] = (uint32_t) total;
  }
  if (t + 1 == total || flags[t + 1] != 0)
  {
    // the running maximum at the last hit of a merged region is its right
    // end: everything in front of the region ends to the left of it
    const uint64_t a = ends[t], b = (flags[t] != 0) ? 0 : prev[t];
    rhi[r] = (POS) ((a > b ? a : b) & mask);
  }
}

// verifyedistlongmatch / verifyedistshortmatch for one merged region.
// COUNT: counts[r] = start positions found; else writes them (descending,
// as the reference reports them) behind offsets[r].
template <int W, bool COUNT, typename POS>
__global__ void __launch_bounds__(VSA_BLOCK)
k_apm_verify_edist(const uint8_t *__restrict__ tis, const DevQueries qs,
                   const uint32_t *__restrict__ qk, uint64_t nregions,
                   const uint32_t *__restrict__ rq,
                   const POS *__restrict__ rlo,
                   const POS *__restrict__ rhi,
                   uint64_t *__restrict__ counts,
                   const uint64_t *__restrict__ offsets,
                   POS *__restrict__ hitpos,
                   uint32_t *__restrict__ hitregion)
{
  const uint64_t r = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (r >= nregions)
  {
    return;
  }
  const uint32_t q = rq[r], k = qk[q];
  const uint8_t *pattern;
  uint32_t m;
  apm_query(qs, q, pattern, m);
  ApmColumn<W> col;
  col.init(pattern, m, true, m > 32); // ISLARGEPATTERN4, splitesaapm.c:254
  const int64_t lo = rlo[r];
  int64_t t = rhi[r];
  uint64_t found = 0, slot = COUNT ? 0 : offsets[r];
  while (t >= lo)
  {
    // the 8 symbols ending at t (the text has 64 bytes of padding in front)
    const uint64_t w8 = vsa_load8(tis + t - 7);
    const int cnt = (t - lo + 1 < 8) ? (int) (t - lo + 1) : 8;
    for (int j = 0; j < cnt; j++)
    {
      const uint8_t c = (uint8_t) (w8 >> (8 * (7 - j)));
      if (c == VSA_SEPARATOR)
      {
        col.reset();
      } else
      {
        col.template step<0>(c);
        if (col.score <= k)
        {
          if (!COUNT)
          {
            hitpos[slot] = (POS) (t - j);
            hitregion[slot] = (uint32_t) r;
            slot++;
          }
          found++;
        }
      }
    }
    t -= cnt;
  }
  if (COUNT)
  {
    counts[r] = found;
  }
}

// edistprocessstartpos: the longest, best-distance prefix behind a start
// position, at most regionmaxlength symbols (approxcompl.c:14-66)
template <int W, typename POS>
__global__ void __launch_bounds__(VSA_BLOCK)
k_apm_longest(const uint8_t *__restrict__ tis, const DevQueries qs,
              const uint32_t *__restrict__ qk, uint64_t nhits,
              const POS *__restrict__ hitpos,
              const uint32_t *__restrict__ hitregion,
              const uint32_t *__restrict__ rq,
              const POS *__restrict__ rlo,
              const POS *__restrict__ rhi, vsa_match *__restrict__ out)
{
  const uint64_t h = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (h >= nhits)
  {
    return;
  }
  const uint32_t r = hitregion[h], q = rq[r], k = qk[q];
  const uint8_t *pattern;
  uint32_t m;
  apm_query(qs, q, pattern, m);
  // splitesaapm.c:254-261: min(m + k, width of the region)
  uint32_t vlen = m + k;
  const uint64_t width = (uint64_t) rhi[r] - (uint64_t) rlo[r] + 1;
  if (vlen > width)
  {
    vlen = (uint32_t) width;
  }
  uint32_t bestlen, bestdist;
  apm_longest_prefix<W>(pattern, m, tis + hitpos[h], vlen, bestlen, bestdist);
  vsa_match mt;
  mt.length = bestlen;
  mt.dbstart = hitpos[h];
  mt.queryseq = (uint64_t) q + qs.seqoffset;
  mt.querystart = bestdist;
  out[h] = mt;
}

// verifyhammingmatch, splitesaapm.c:198-250, for one merged region
template <bool COUNT, typename POS>
__global__ void __launch_bounds__(VSA_BLOCK)
k_apm_verify_hamming(const uint8_t *__restrict__ tis, const DevQueries qs,
                     const uint32_t *__restrict__ qk, uint64_t nregions,
                     const uint32_t *__restrict__ rq,
                     const POS *__restrict__ rlo,
                     const POS *__restrict__ rhi,
                     uint64_t *__restrict__ counts,
                     const uint64_t *__restrict__ offsets,
                     vsa_match *__restrict__ out)
{
  const uint64_t r = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (r >= nregions)
  {
    return;
  }
  const uint32_t q = rq[r], k = qk[q];
  const uint8_t *pattern;
  uint32_t m;
  apm_query(qs, q, pattern, m);
  const int64_t lo = rlo[r];
  int64_t t = (int64_t) rhi[r] - (int64_t) m + 1;
  uint64_t found = 0, slot = COUNT ? 0 : offsets[r];
  const uint64_t H = 0x8080808080808080ull, L = 0x7F7F7F7F7F7F7F7Full;
  while (t >= lo)
  {
    if (tis[t] == VSA_SEPARATOR)
    {
      t -= (int64_t) m + 1; // the reference passes m + 1 positions here
      continue;
    }
    uint32_t mm = 0;
    bool sep = false;
    for (uint32_t i = 0; i < m && !sep && mm <= k; i += 8)
    {
      const uint64_t tw = vsa_load8(tis + t + i), pw = vsa_load8(pattern + i);
      const uint32_t valid = (m - i < 8) ? m - i : 8;
      const uint64_t vmask = (valid == 8) ? ~0ull : ((1ull << (8 * valid)) - 1);
      const uint64_t x = (tw ^ pw) & vmask;
      const uint64_t ns = ~tw; // a zero byte of ~tw is a separator
      const uint64_t notsep = (((ns & L) + L) | ns) & H;
      sep = ((~notsep & H) & vmask) != 0;
      mm += (uint32_t) __builtin_popcountll((((x & L) + L) | x) & H);
    }
    if (!sep && mm <= k)
    {
      if (!COUNT)
      {
        vsa_match mt;
        mt.length = m;
        mt.dbstart = (uint64_t) t;
        mt.queryseq = (uint64_t) q + qs.seqoffset;
        mt.querystart = mm;
        out[slot++] = mt;
      }
      found++;
    }
    t--;
  }
  if (COUNT)
  {
    counts[r] = found;
  }
}

// ---- the fast path for edit distance (no special symbol in any query,
// thresholds <= 3) ------------------------------------------------------------
//
// An occurrence with <= k errors contains one of the >= k+1 pieces without
// error, so it starts within k positions of (piece hit - piece offset) = the
// left end of that hit's region + k.  Instead of scanning a merged region
// symbol by symbol, only the start positions lo .. lo + 2k behind the left
// ends of its hits are examined, each by a banded global alignment (cells
// with |row - column| <= k; everything <= k is exact there).  The last row
// of the band holds D[m][j] for j = m-k .. m+k, which answers both of the
// reference's questions: "is there a prefix of the text at this start within
// k errors that ends inside the region" (the verification,
// splitesaapm.c:44-196) and "which prefix of at most regionmaxlength symbols
// has the best distance, the longest among equals" (longestmatch.c:18-71).

// start positions of region r, descending, without duplicates
template <bool COUNT, typename POS>
__global__ void __launch_bounds__(VSA_BLOCK)
k_apm_candidates(const uint64_t *__restrict__ keys, uint32_t pbits,
                 const uint32_t *__restrict__ qk, uint64_t nregions,
                 const uint32_t *__restrict__ rq,
                 const uint32_t *__restrict__ rfirst,
                 uint64_t *__restrict__ counts,
                 const uint64_t *__restrict__ offsets,
                 POS *__restrict__ candpos,
                 uint32_t *__restrict__ candregion)
{
  const uint64_t r = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (r >= nregions)
  {
    return;
  }
  const uint32_t k = qk[rq[r]];
  uint64_t found = 0, slot = COUNT ? 0 : offsets[r];
  int64_t bound = INT64_MAX; // positions >= bound have been taken
  for (int64_t t = (int64_t) rfirst[r + 1] - 1; t >= (int64_t) rfirst[r]; t--)
  {
    const int64_t lo = (int64_t) (keys[t] & ((1ull << pbits) - 1));
    int64_t upper = lo + 2 * (int64_t) k;
    if (upper >= bound)
    {
      upper = bound - 1;
    }
    for (int64_t p = upper; p >= lo; p--)
    {
      if (!COUNT)
      {
        candpos[slot] = (POS) p;
        candregion[slot] = (uint32_t) r;
        slot++;
      }
      found++;
    }
    if (lo < bound)
    {
      bound = lo;
    }
  }
  if (COUNT)
  {
    counts[r] = found;
  }
}

#define VSA_APM_BANDK 3 // the band's text window is one 8-byte load

// one row of the band: cells e = 0 .. 2K, column j = i + e - K.  CHECKED:
// rows 1 .. K, where columns <= 0 occur.
// LIMITED = false: every column of the row lies in front of `limit` (the
// caller has looked), no test per cell.
template <int K, bool CHECKED, bool LIMITED = true>
__device__ __forceinline__ void
apm_bandrow(uint32_t (&band)[2 * K + 1], uint32_t i, uint8_t pc, uint64_t tw,
            uint32_t limit, uint32_t INF)
{
  const bool pcwild = pc == VSA_WILDCARD;
#pragma unroll
  for (int e = 0; e < 2 * K + 1; e++)
  {
    const int j = (int) i + e - K;
    const uint8_t c = (uint8_t) (tw >> (8 * e));
    uint32_t v;
    if (CHECKED && j < 0)
    {
      v = INF;
    } else if (CHECKED && j == 0)
    {
      v = (i < INF) ? i : INF;
    } else if (LIMITED && (uint32_t) (j - 1) >= limit) // behind vlen or a
    {                                                   // separator
      v = INF;
    } else
    {
      v = band[e] + ((pc != c || pcwild) ? 1u : 0u);
      if (e + 1 < 2 * K + 1)
      {
        const uint32_t up = band[e + 1] + 1;
        v = (up < v) ? up : v;
      }
      if (e > 0)
      {
        const uint32_t lf = band[e - 1] + 1;
        v = (lf < v) ? lf : v;
      }
      v = (v < INF) ? v : INF;
    }
    band[e] = v;
  }
}

// K = the largest threshold of the batch: a band wider than a query's own
// threshold k is as exact (cells beyond |row - column| <= k hold values > k,
// which are clamped to k + 1 either way)
template <int K, typename POS>
__global__ void __launch_bounds__(VSA_BLOCK)
k_apm_banded(const uint8_t *__restrict__ tis, uint64_t n,
             const DevQueries qs, const uint32_t *__restrict__ qk,
             uint64_t ncand, const POS *__restrict__ candpos,
             const uint32_t *__restrict__ candregion,
             const uint32_t *__restrict__ rq,
             const POS *__restrict__ rlo,
             const POS *__restrict__ rhi, vsa_match *__restrict__ out,
             uint8_t *__restrict__ keep)
{
  const uint64_t h = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (h >= ncand)
  {
    return;
  }
  const uint32_t r = candregion[h], q = rq[r], k = qk[q];
  const uint64_t p = candpos[h];
  const uint8_t *pattern;
  uint32_t m;
  apm_query(qs, q, pattern, m);
  const uint64_t width = (uint64_t) rhi[r] - (uint64_t) rlo[r] + 1;
  const uint32_t vlen =
      (m + k > width) ? (uint32_t) width : m + k; // regionmaxlength
  // columns inside the region (what matters is whether it reaches m + K)
  const uint64_t inregion = (uint64_t) rhi[r] - p + 1;
  const uint32_t jverify =
      inregion > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t) inregion;
  const uint32_t INF = k + 1;
  constexpr int NB = 2 * K + 1;
  // the window of one row: NB text symbols
  const uint64_t winmask = (NB == 8) ? ~0ull : ((1ull << (8 * NB)) - 1);
  const uint64_t H8 = 0x8080808080808080ull, L8 = 0x7F7F7F7F7F7F7F7Full;
  uint32_t band[NB];
  uint32_t limit = vlen; // columns 1 .. limit can be used

  // row 0: D[0][j] = j; band cell e of row i is column j = i + e - K
#pragma unroll
  for (int e = 0; e < NB; e++)
  {
    const int j = e - K;
    band[e] = (j >= 0 && (uint32_t) j < INF) ? (uint32_t) j : INF;
  }
  // eight rows at a time: eight pattern symbols and the sixteen text symbols
  // their windows lie in come with one load each (a load per row and its
  // separator test were a third of the work)
  bool dead = false;
  for (uint32_t i0 = 1; i0 <= m && !dead; i0 += 8)
  {
    const uint64_t pw = vsa_load8(pattern + i0 - 1);
    // nothing within k errors any more: this start position is dead
    bool alive = false;
#pragma unroll
    for (int e = 0; e < NB; e++)
    {
      alive |= band[e] < INF;
    }
    if (!alive)
    {
      break;
    }
    // text symbols of columns i-K .. i+K of row i (column j is text position
    // p+j-1; the text has 64 bytes of padding on both sides; behind the end
    // of the text every column is beyond a separator and the symbols are not
    // looked at: keep the load inside the padding)
    int64_t toff = (int64_t) p + (int64_t) i0 - K - 1;
    if (toff > (int64_t) n)
    {
      toff = (int64_t) n;
    }
    const vsa_u128 tx = vsa_load16(tis + toff);
    // 0x80 in every byte that is a separator
    const uint64_t nlo = ~tx.lo, nhi = ~tx.hi;
    const uint64_t seplo = ~((((nlo & L8) + L8) | nlo)) & H8,
                   sephi = ~((((nhi & L8) + L8) | nhi)) & H8;
#pragma unroll
    for (uint32_t r = 0; r < 8; r++)
    {
      const uint32_t i = i0 + r;
      if (i > m)
      {
        dead = true; // rows are exhausted
        break;
      }
      const uint8_t pc = (uint8_t) (pw >> (8 * r));
      const uint64_t tw =
          r == 0 ? tx.lo : ((tx.lo >> (8 * r)) | (tx.hi << (64 - 8 * r)));
      // a separator in the window ends the usable columns in front of it
      uint64_t sep = (r == 0 ? seplo
                             : ((seplo >> (8 * r)) | (sephi << (64 - 8 * r)))) &
                     winmask;
      if (i <= (uint32_t) K)
      {
        sep &= ~0ull << (8 * (K + 1 - (int) i)); // columns <= 0: not text of p
      }
      if (sep != 0)
      {
        const int e = __builtin_ctzll(sep) >> 3;
        const int j = (int) i + e - K;
        if (j >= 1 && (uint32_t) (j - 1) < limit)
        {
          limit = (uint32_t) (j - 1);
        }
      }
      if (i <= (uint32_t) K)
      {
        apm_bandrow<K, true>(band, i, pc, tw, limit, INF);
      } else if (i + K <= limit)
      {
        // the usual row: columns i-K .. i+K all usable
        apm_bandrow<K, false, false>(band, i, pc, tw, limit, INF);
      } else
      {
        apm_bandrow<K, false>(band, i, pc, tw, limit, INF);
      }
    }
  }
  uint32_t bestlen = 0, bestdist = m, hitmin = INF;
#pragma unroll
  for (int e = 0; e < NB; e++)
  {
    const int j = (int) m + e - K;
    if (j >= 1)
    {
      const uint32_t sc = band[e];
      if ((uint32_t) j <= jverify && sc < hitmin)
      {
        hitmin = sc;
      }
      if (sc <= k && bestdist >= sc) // UPDATELENGTHANDSCORE
      {
        bestlen = (uint32_t) j;
        bestdist = sc;
      }
    }
  }
  vsa_match mt;
  mt.length = bestlen;
  mt.dbstart = p;
  mt.queryseq = (uint64_t) q + qs.seqoffset;
  mt.querystart = bestdist;
  out[h] = mt;
  keep[h] = (hitmin <= k) ? 1 : 0;
}

struct MaxU64
{
  __device__ uint64_t operator()(uint64_t a, uint64_t b) const
  {
    return a > b ? a : b;
  }
};

// the host-side plan of a batch: thresholds and piece geometry per query
struct ApmPlan
{
  std::vector<uint32_t> k, splitlen;
  std::vector<uint64_t> piecebase; // nq + 1
  uint64_t qlimit;                 // queries in front of the first failure
  uint64_t failk, failm;           // threshold >= patternlength at qlimit
  uint32_t maxm;
  bool allexact;
  // every query has the same length (the usual read batch): one threshold,
  // one piece length, `upieces` pieces per query, and the three vectors stay
  // empty -- filling and uploading them cost 70 ms for 10 M reads, twice the
  // whole search
  bool uniform;
  uint32_t uk, usplitlen, upieces;
  // reads of different lengths, all of them plannable: threshold, piece
  // length and number of pieces per LENGTH (tables of maxm + 1 entries); the
  // per-query arrays are filled on the device from the lengths there
  bool bylength;
  std::vector<uint32_t> tk, tsplitlen, tpieces;
  uint64_t totalpieces;
  uint64_t npieces(uint64_t nq) const
  {
    return uniform ? nq * upieces : (bylength ? totalpieces : piecebase[nq]);
  }
  uint32_t maxk(uint64_t nq) const // the largest threshold
  {
    if (uniform)
    {
      return uk;
    }
    return bylength ? *std::max_element(tk.begin(), tk.end())
                    : *std::max_element(k.begin(), k.begin() + nq);
  }
};

#define VSA_APM_TABLEMAX 4096u

// how many queries have which length (lengths <= VSA_APM_TABLEMAX)
__global__ void __launch_bounds__(VSA_BLOCK)
k_apm_lengthhist(const uint64_t *__restrict__ length, uint64_t nq,
                 uint32_t maxlen, unsigned long long *__restrict__ hist)
{
  const uint64_t q = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (q < nq)
  {
    const uint64_t m = length[q];
    atomicAdd(hist + (m <= maxlen ? m : maxlen), 1ull);
  }
}

// the plan arrays from the per-length tables; pieces[q] for the scan that
// gives piecebase
__global__ void __launch_bounds__(VSA_BLOCK)
k_apm_filltable(const uint64_t *__restrict__ length, uint64_t nq,
                const uint32_t *__restrict__ tk,
                const uint32_t *__restrict__ tsplitlen,
                const uint32_t *__restrict__ tpieces,
                uint32_t *__restrict__ k, uint32_t *__restrict__ splitlen,
                uint64_t *__restrict__ pieces)
{
  const uint64_t q = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (q < nq)
  {
    const uint64_t m = length[q];
    k[q] = tk[m];
    splitlen[q] = tsplitlen[m];
    pieces[q] = tpieces[m];
  }
  if (q == nq)
  {
    pieces[q] = 0;
  }
}

// the plan arrays of a uniform batch, written where they are used
__global__ void __launch_bounds__(VSA_BLOCK)
k_apm_fillplan(uint32_t *__restrict__ k, uint32_t *__restrict__ splitlen,
               uint64_t *__restrict__ piecebase, uint64_t nq, uint32_t uk,
               uint32_t usplitlen, uint32_t upieces)
{
  const uint64_t q = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (q < nq)
  {
    k[q] = uk;
    splitlen[q] = usplitlen;
  }
  if (q <= nq)
  {
    piecebase[q] = q * upieces;
  }
}

// Thresholds read by read instead of one rule for the batch: the second pass
// of a "best of" job (approx_bestof, esa_search.hip) sets this around its call
// of approx_batch; entry q = the threshold of query q of THAT batch.
static thread_local const uint32_t *apm_explicitk = nullptr;

// 0 ok, VSA_NOT_COVERED with a message otherwise
static int apm_plan(const vsa_index *index, const vsa_queries *queries,
                    bool doedist, uint64_t distvalue, bool percent,
                    ApmPlan &plan)
{
  const uint64_t nq = queries->nq;
  uint64_t lastm = ~0ull, lastk = 0, lastsplit = 0, exact = 0;

  plan.qlimit = nq;
  plan.maxm = 0;
  plan.failk = plan.failm = 0;
  plan.uniform = false;
  plan.bylength = false;
  plan.totalpieces = 0;
  plan.uk = plan.usplitlen = plan.upieces = 0;
  plan.k.clear();
  plan.splitlen.clear();
  plan.piecebase.clear();
  if (!queries->uniform && nq > 4096 && apm_explicitk == nullptr &&
      queries->maxlength <= VSA_APM_TABLEMAX)
  {
    // many reads of a few lengths: plan per length.  Anything unusual (a
    // threshold of 0 or beyond the length, a length the engine does not
    // cover) goes to the loop below, which knows which query is the first.
    const uint32_t maxlen = (uint32_t) queries->maxlength;
    std::vector<unsigned long long> present(maxlen + 1, 0);
    DevBuf dhist;
    vsa_dev_set_stream(index->stream);
    if (vsa_set_device(index->device) != 0 ||
        dhist.alloc(((size_t) maxlen + 1) * 8))
    {
      return -100;
    }
    VSA_HIP(hipMemsetAsync(dhist.p, 0, ((size_t) maxlen + 1) * 8,
                           index->stream));
    k_apm_lengthhist<<<gridfor(nq), VSA_BLOCK, 0, index->stream>>>(
        queries->length, nq, maxlen, dhist.as<unsigned long long>());
    VSA_HIP(hipGetLastError());
    VSA_HIP(hipMemcpyAsync(present.data(), dhist.p,
                           ((size_t) maxlen + 1) * 8, hipMemcpyDeviceToHost,
                           index->stream));
    VSA_HIP(hipStreamSynchronize(index->stream));
    plan.tk.assign(maxlen + 1, 0);
    plan.tsplitlen.assign(maxlen + 1, 0);
    plan.tpieces.assign(maxlen + 1, 0);
    bool plain = true;
    for (uint64_t m = 0; m <= maxlen && plain; m++)
    {
      if (present[m] == 0)
      {
        continue;
      }
      const uint64_t k = percent ? (m * distvalue) / 100 : distvalue;
      if (k == 0 || k >= m || m > 64 * VSA_APM_MAXWORDS)
      {
        plain = false;
        break;
      }
      const uint64_t splitsize =
          apm_getoptsplit(doedist, 10, index->numofchars, index->n, m, k);
      if (splitsize <= 1 || k / splitsize != 0 || m / splitsize < index->pl)
      {
        plain = false;
        break;
      }
      const uint64_t splitlen = m / splitsize;
      plan.tk[m] = (uint32_t) k;
      plan.tsplitlen[m] = (uint32_t) splitlen;
      plan.tpieces[m] = (uint32_t) (m / splitlen);
      plan.totalpieces += present[m] * (m / splitlen);
      plan.maxm = (uint32_t) m;
    }
    if (plain)
    {
      plan.bylength = true;
      plan.allexact = false;
      return 0;
    }
    plan.maxm = 0;
    plan.totalpieces = 0;
  }
  // a batch of equal lengths is planned through its first query alone
  const uint64_t nplan =
      (queries->uniform && nq > 0 && apm_explicitk == nullptr) ? 1 : nq;
  plan.k.assign(nplan, 0);
  plan.splitlen.assign(nplan, 0);
  plan.piecebase.assign(nplan + 1, 0);
  for (uint64_t q = 0; q < nplan; q++)
  {
    const uint64_t m = queries->uniform ? queries->maxlength
                                        : queries->hlength[q];
    const uint64_t k = apm_explicitk != nullptr
                           ? apm_explicitk[q]
                           : (percent ? (m * distvalue) / 100 : distvalue);
    plan.piecebase[q + 1] = plan.piecebase[q];
    if (k == 0)
    {
      exact++;
      continue;
    }
    if (k >= m)
    {
      // splitesaapm.c:496-501: stops the run at this query
      plan.qlimit = q;
      plan.failk = k;
      plan.failm = m;
      break;
    }
    if (m != lastm || k != lastk)
    {
      lastsplit = apm_getoptsplit(doedist, 10, index->numofchars, index->n, m,
                                  k);
      lastm = m;
      lastk = k;
    }
    const uint64_t splitsize = lastsplit;
    if (splitsize <= 1 || k / splitsize != 0)
    {
      VSA_ERROR("approximate search of query %lu (length %lu, threshold %lu: "
                "%lu pieces with threshold %lu) is not covered by the GPU "
                "engine", (unsigned long) q, (unsigned long) m,
                (unsigned long) k, (unsigned long) splitsize,
                (unsigned long) (splitsize ? k / splitsize : 0));
      return VSA_NOT_COVERED;
    }
    const uint64_t splitlen = m / splitsize;
    if (splitlen < index->pl || m > 64 * VSA_APM_MAXWORDS)
    {
      VSA_ERROR("approximate search of query %lu (length %lu, pieces of "
                "length %lu, prefixlength %lu) is not covered by the GPU "
                "engine", (unsigned long) q, (unsigned long) m,
                (unsigned long) splitlen, (unsigned long) index->pl);
      return VSA_NOT_COVERED;
    }
    plan.k[q] = (uint32_t) k;
    plan.splitlen[q] = (uint32_t) splitlen;
    plan.piecebase[q + 1] += m / splitlen; // offsets 0, sl, .. while <= m-sl
    if (m > plan.maxm)
    {
      plan.maxm = (uint32_t) m;
    }
  }
  if (nplan != nq)
  {
    if (plan.qlimit == 0)
    {
      // threshold >= pattern length: the run stops at the first query
      plan.k.clear();
      plan.splitlen.clear();
      plan.piecebase.assign(1, 0);
    } else
    {
      plan.uniform = true;
      plan.uk = plan.k[0];
      plan.usplitlen = plan.splitlen[0];
      plan.upieces = (uint32_t) plan.piecebase[1];
      plan.qlimit = nq;
      exact = exact != 0 ? nq : 0;
      plan.k.clear();
      plan.splitlen.clear();
      plan.piecebase.clear();
    }
  }
  plan.allexact = exact == nq;
  if (exact != 0 && !plan.allexact)
  {
    VSA_ERROR("a batch that mixes thresholds 0 and > 0 is not covered by the "
              "GPU engine");
    return VSA_NOT_COVERED;
  }
  return 0;
}

// ---- the stages of the approximate search ---------------------------------
// run_approx (below) and run_approx_tree (approx_tree.inc) are lists of these.

// fn(W): W = std::integral_constant<int, words>, the 64-bit words of the
// longest pattern (1 .. VSA_APM_MAXWORDS)
template <typename Fn>
void withwords(int words, Fn &&fn)
{
  switch (words)
  {
  case 1: return fn(std::integral_constant<int, 1>());
  case 2: return fn(std::integral_constant<int, 2>());
  case 3: return fn(std::integral_constant<int, 3>());
  case 4: return fn(std::integral_constant<int, 4>());
  case 5: return fn(std::integral_constant<int, 5>());
  case 6: return fn(std::integral_constant<int, 6>());
  case 7: return fn(std::integral_constant<int, 7>());
  default: return fn(std::integral_constant<int, 8>());
  }
}

// fn(K): K = std::integral_constant<int, maxk>, the band of the alignment
// (1 .. VSA_APM_BANDK)
template <typename Fn>
void withband(uint32_t maxk, Fn &&fn)
{
  switch (maxk)
  {
  case 1: return fn(std::integral_constant<int, 1>());
  case 2: return fn(std::integral_constant<int, 2>());
  default: return fn(std::integral_constant<int, 3>());
  }
}

// sort keys: query number << pbits | text position (32 bits where the
// tables are 32 bits wide: the layout of rounds 1 and 2)
template <typename IDX>
int apm_positionbits(const vsa_index *index, const vsa_queries *queries,
                     uint64_t maxqueries, uint32_t *pbits)
{
  *pbits = sizeof(IDX) == 4 ? 32u : bitsfor(index->n);
  if (queries->nq >= maxqueries || *pbits + bitsfor(queries->nq) > 64)
  {
    VSA_ERROR("approximate search: a batch of %lu reads on a text of %lu "
              "symbols is not covered by the GPU engine",
              (unsigned long) queries->nq, (unsigned long) index->n);
    return VSA_NOT_COVERED;
  }
  return 0;
}

// The plan of a batch on the device and the pieces its queries are cut into.
struct ApmPieces
{
  DevBuf k, splitlen, piecebase;     // per query; piecebase has nq + 1 entries
  DevBuf start, len, query, poffset; // per piece
  int alloc(uint64_t nq, uint64_t npieces)
  {
    return (k.alloc(nq * 4) || splitlen.alloc(nq * 4) ||
            piecebase.alloc((nq + 1) * 8) || start.alloc(npieces * 8) ||
            len.alloc(npieces * 8) || query.alloc(npieces * 4) ||
            poffset.alloc(npieces * 4))
               ? -100
               : 0;
  }
  // the plan arrays from vectors with an entry per query
  int upload(const std::vector<uint32_t> &hk,
             const std::vector<uint32_t> &hsplitlen,
             const std::vector<uint64_t> &hpiecebase, uint64_t nq,
             hipStream_t stream)
  {
    VSA_HIP(hipMemcpyAsync(k.p, hk.data(), nq * 4, hipMemcpyHostToDevice,
                           stream));
    VSA_HIP(hipMemcpyAsync(splitlen.p, hsplitlen.data(), nq * 4,
                           hipMemcpyHostToDevice, stream));
    VSA_HIP(hipMemcpyAsync(piecebase.p, hpiecebase.data(), (nq + 1) * 8,
                           hipMemcpyHostToDevice, stream));
    return 0;
  }
  // the pieces from the plan arrays
  int cut(const DevQueries &qs, uint64_t nq, hipStream_t stream)
  {
    k_apm_pieces<<<gridfor(nq), VSA_BLOCK, 0, stream>>>(
        qs, nq, splitlen.as<uint32_t>(), piecebase.as<uint64_t>(),
        start.as<uint64_t>(), len.as<uint64_t>(), query.as<uint32_t>(),
        poffset.as<uint32_t>());
    VSA_HIP(hipGetLastError());
    return 0;
  }
};

// the plan arrays of an ApmPlan, in the way the plan was made, and the pieces
static int apm_pieces(const ApmPlan &plan, const DevQueries &qs, uint64_t nq,
                      hipStream_t stream, ApmPieces &pc)
{
  if (plan.bylength)
  {
    const size_t tn = plan.tk.size();
    DevBuf dtk, dtsplit, dtpieces, dpieces;
    uint64_t npieces = 0;
    if (dtk.alloc(tn * 4) || dtsplit.alloc(tn * 4) || dtpieces.alloc(tn * 4) ||
        dpieces.alloc((nq + 1) * 8))
    {
      return -100;
    }
    VSA_HIP(hipMemcpyAsync(dtk.p, plan.tk.data(), tn * 4,
                           hipMemcpyHostToDevice, stream));
    VSA_HIP(hipMemcpyAsync(dtsplit.p, plan.tsplitlen.data(), tn * 4,
                           hipMemcpyHostToDevice, stream));
    VSA_HIP(hipMemcpyAsync(dtpieces.p, plan.tpieces.data(), tn * 4,
                           hipMemcpyHostToDevice, stream));
    k_apm_filltable<<<gridfor(nq + 1), VSA_BLOCK, 0, stream>>>(
        qs.length, nq, dtk.as<uint32_t>(), dtsplit.as<uint32_t>(),
        dtpieces.as<uint32_t>(), pc.k.as<uint32_t>(),
        pc.splitlen.as<uint32_t>(), dpieces.as<uint64_t>());
    VSA_HIP(hipGetLastError());
    // (synchronises: the tables are host vectors of this call, and the copies
    // are done before they can go away)
    if (exclusive_sum(dpieces.as<uint64_t>(), pc.piecebase.as<uint64_t>(), nq,
                      stream, &npieces))
    {
      return -100;
    }
  } else if (plan.uniform)
  {
    k_apm_fillplan<<<gridfor(nq + 1), VSA_BLOCK, 0, stream>>>(
        pc.k.as<uint32_t>(), pc.splitlen.as<uint32_t>(),
        pc.piecebase.as<uint64_t>(), nq, plan.uk, plan.usplitlen,
        plan.upieces);
    VSA_HIP(hipGetLastError());
  } else if (pc.upload(plan.k, plan.splitlen, plan.piecebase, nq, stream))
  {
    return -100;
  }
  return pc.cut(qs, nq, stream);
}

// A1: exact search of every piece = the K1 kernel on a batch of pieces;
// left[p], count[p] = the suffix array interval of piece p
template <typename IDX>
int apm_searchpieces(const DevIndex<IDX> &ix, const DevQueries &qs,
                     ApmPieces &pc, uint64_t npieces, Timer &tsearch,
                     hipStream_t stream, uint64_t *left, uint64_t *count)
{
  DevQueries ps = qs;
  ps.start = pc.start.as<uint64_t>();
  ps.length = pc.len.as<uint64_t>();
  ps.nq = npieces;
  ps.uniformlen = 0;
  ps.dense = 0;
  VSA_HIP(hipMemsetAsync(count + npieces, 0, 8, stream));
  tsearch.start();
  if constexpr (sizeof(IDX) == 4)
  {
    if (ix.esa8 != nullptr)
    {
      k_complete_search<IDX, true><<<gridfor(npieces), VSA_BLOCK, 0, stream>>>(
          ix, ps, npieces, left, count);
    } else
    {
      k_complete_search<IDX, false>
          <<<gridfor(npieces), VSA_BLOCK, 0, stream>>>(ix, ps, npieces, left,
                                                       count);
    }
  } else
  {
    k_complete_search<IDX, false><<<gridfor(npieces), VSA_BLOCK, 0, stream>>>(
        ix, ps, npieces, left, count);
  }
  tsearch.stop();
  VSA_HIP(hipGetLastError());
  return 0;
}

// What the pieces of a batch have hit: source i (a piece; an interval of the
// tree search in approx_tree.inc) stands for the suffixes left[i],
// left[i] + 1, .. of the suffix array, offsets[i + 1] - offsets[i] of them,
// found for query[i] at offset poffset[i] of its pattern.
struct ApmHits
{
  const uint64_t *left, *offsets;
  const uint32_t *query, *poffset;
  uint64_t nsources, total; // total = offsets[nsources], > 0
};

// A2: the regions of the text that have to be verified, one stretch per hit,
// merged where they overlap, in the order (query, left end).
struct ApmRegions
{
  uint64_t n = 0;
  uint32_t pbits;      // sort keys: query << pbits | text position
  DevBuf rq, rlo, rhi; // per region: its query, its first and last position
  DevBuf rfirst;       // n + 1: the first hit of a region in keys
  DevBuf keys;         // the keys of the hits, sorted
};

// segments: the sources of query q are segments[q] .. segments[q + 1] - 1, so
// that the hits can be sorted inside the queries (radix sort of the whole list
// only if a query has too many); nullptr: radix sort
template <typename IDX>
int apm_regions(const DevIndex<IDX> &ix, const DevQueries &qs, uint64_t nq,
                const ApmHits &hits, const uint32_t *dk, bool doedist,
                const uint64_t *segments, hipStream_t stream, ApmRegions &rg)
{
  const uint64_t total = hits.total;
  const uint32_t pbits = rg.pbits;
  DevBuf keys, his, his2, ends, prev, flags, rank, temp;
  if (keys.alloc(total * 8) || rg.keys.alloc(total * 8) ||
      his.alloc(total * sizeof(IDX)) || his2.alloc(total * sizeof(IDX)) ||
      ends.alloc(total * 8) || prev.alloc(total * 8) ||
      flags.alloc(total * 4) || rank.alloc(total * 4))
  {
    return -100;
  }
  k_apm_regions<IDX, IDX><<<gridfor(hits.nsources), VSA_BLOCK, 0, stream>>>(
      ix, qs, hits.nsources, hits.left, hits.offsets, total, hits.query,
      hits.poffset, dk, doedist, pbits, keys.as<uint64_t>(), his.as<IDX>());
  VSA_HIP(hipGetLastError());
  // sorted by (query, left end): inside the queries where that will do
  uint64_t bigsegment = 1;
  if (segments != nullptr)
  {
    // (the first word of flags, not yet in use, says whether it did)
    VSA_HIP(hipMemsetAsync(flags.p, 0, 4, stream));
    k_apm_sortsegments<<<gridfor(nq), VSA_BLOCK, 0, stream>>>(
        segments, hits.offsets, nq, keys.as<uint64_t>(), his.as<IDX>(),
        flags.as<unsigned int>());
    VSA_HIP(hipGetLastError());
    const Fetch f = {flags.p, 4};
    if (fetchwords(stream, &f, 1, &bigsegment))
    {
      return -100;
    }
  }
  if (bigsegment != 0)
  {
    const unsigned int endbit = pbits + bitsfor(nq);
    VSA_HIP(rocprim_run(temp, [&](void *p, size_t &tb) {
      return rocprim::radix_sort_pairs(
          p, tb, keys.as<uint64_t>(), rg.keys.as<uint64_t>(), his.as<IDX>(),
          his2.as<IDX>(), (size_t) total, 0u, endbit, stream);
    }));
  } else
  {
    // in place: the sorted list is the input list
    std::swap(keys.p, rg.keys.p);
    std::swap(his.p, his2.p);
  }
  // running maximum of the right ends: a hit that starts behind it starts a
  // new region
  k_apm_rightends<<<gridfor(total), VSA_BLOCK, 0, stream>>>(
      rg.keys.as<uint64_t>(), his2.as<IDX>(), total, pbits,
      ends.as<uint64_t>());
  VSA_HIP(hipGetLastError());
  VSA_HIP(rocprim_run(temp, [&](void *p, size_t &tb) {
    return rocprim::exclusive_scan(p, tb, ends.as<uint64_t>(),
                                   prev.as<uint64_t>(), (uint64_t) 0,
                                   (size_t) total, MaxU64(), stream);
  }));
  k_apm_flags<<<gridfor(total), VSA_BLOCK, 0, stream>>>(
      rg.keys.as<uint64_t>(), prev.as<uint64_t>(), total, pbits,
      flags.as<uint32_t>());
  VSA_HIP(hipGetLastError());
  VSA_HIP(rocprim_run(temp, [&](void *p, size_t &tb) {
    return rocprim::inclusive_scan(p, tb, flags.as<uint32_t>(),
                                   rank.as<uint32_t>(), (size_t) total,
                                   rocprim::plus<uint32_t>(), stream);
  }));
  uint32_t hlast = 0;
  VSA_HIP(hipMemcpyAsync(&hlast, rank.as<uint32_t>() + total - 1, 4,
                         hipMemcpyDeviceToHost, stream));
  VSA_HIP(hipStreamSynchronize(stream));
  rg.n = hlast;
  if (rg.rq.alloc(rg.n * 4) || rg.rlo.alloc(rg.n * sizeof(IDX)) ||
      rg.rhi.alloc(rg.n * sizeof(IDX)) || rg.rfirst.alloc((rg.n + 1) * 4))
  {
    return -100;
  }
  k_apm_writeregions<<<gridfor(total), VSA_BLOCK, 0, stream>>>(
      rg.keys.as<uint64_t>(), ends.as<uint64_t>(), prev.as<uint64_t>(),
      flags.as<uint32_t>(), rank.as<uint32_t>(), total, pbits,
      rg.rq.as<uint32_t>(), rg.rlo.as<IDX>(), rg.rhi.as<IDX>(),
      rg.rfirst.as<uint32_t>());
  VSA_HIP(hipGetLastError());
  return 0;
}

// the longest match at each of n start positions (hitpos, in region
// hitregion): one record per position
template <typename IDX>
int apm_longest(const uint8_t *tis, const DevQueries &qs, const uint32_t *dk,
                int words, uint64_t n, const IDX *hitpos,
                const uint32_t *hitregion, const uint32_t *rq, const IDX *rlo,
                const IDX *rhi, vsa_match *out, hipStream_t stream)
{
  withwords(words, [&](auto w) {
    k_apm_longest<decltype(w)::value><<<gridfor(n), VSA_BLOCK, 0, stream>>>(
        tis, qs, dk, n, hitpos, hitregion, rq, rlo, rhi, out);
  });
  VSA_HIP(hipGetLastError());
  return 0;
}

// A3: verification of the regions, count pass then write pass; matches (empty
// on entry; allocated if *nhits > 0) = the matches, in the order of the regions
template <typename IDX>
int apm_verify(const uint8_t *tis, const DevQueries &qs, const uint32_t *dk,
               int words, bool doedist, ApmRegions &rg, hipStream_t stream,
               DevBuf &matches, uint64_t *nhits)
{
  const uint64_t nregions = rg.n;
  DevBuf rcount, roffsets, hitpos, hitregion;
  if (rcount.alloc((nregions + 1) * 8) || roffsets.alloc((nregions + 1) * 8))
  {
    return -100;
  }
  VSA_HIP(hipMemsetAsync(rcount.as<uint64_t>() + nregions, 0, 8, stream));
  auto pass = [&](auto count) {
    constexpr bool COUNT = decltype(count)::value;
    if (doedist)
    {
      withwords(words, [&](auto w) {
        k_apm_verify_edist<decltype(w)::value, COUNT>
            <<<gridfor(nregions), VSA_BLOCK, 0, stream>>>(
                tis, qs, dk, nregions, rg.rq.as<uint32_t>(),
                rg.rlo.as<IDX>(), rg.rhi.as<IDX>(), rcount.as<uint64_t>(),
                roffsets.as<uint64_t>(), hitpos.as<IDX>(),
                hitregion.as<uint32_t>());
      });
    } else
    {
      k_apm_verify_hamming<COUNT><<<gridfor(nregions), VSA_BLOCK, 0, stream>>>(
          tis, qs, dk, nregions, rg.rq.as<uint32_t>(), rg.rlo.as<IDX>(),
          rg.rhi.as<IDX>(), rcount.as<uint64_t>(), roffsets.as<uint64_t>(),
          matches.as<vsa_match>());
    }
    return hipGetLastError();
  };
  VSA_HIP(pass(std::true_type()));
  if (exclusive_sum(rcount.as<uint64_t>(), roffsets.as<uint64_t>(), nregions,
                    stream, nhits))
  {
    return -100;
  }
  if (*nhits == 0)
  {
    return 0;
  }
  if (matches.alloc(*nhits * sizeof(vsa_match)) ||
      (doedist && (hitpos.alloc(*nhits * sizeof(IDX)) ||
                   hitregion.alloc(*nhits * 4))))
  {
    return -100;
  }
  VSA_HIP(pass(std::false_type()));
  // edit distance: the write pass gave the start positions
  return doedist ? apm_longest<IDX>(tis, qs, dk, words, *nhits,
                                    hitpos.as<IDX>(),
                                    hitregion.as<uint32_t>(),
                                    rg.rq.as<uint32_t>(), rg.rlo.as<IDX>(),
                                    rg.rhi.as<IDX>(),
                                    matches.as<vsa_match>(), stream)
                 : 0;
}

// A3 for edit distance with thresholds up to VSA_APM_BANDK: the start
// positions the hits allow (count pass, write pass), a banded alignment at
// each of them (tband; *naligned = how many), and the ones it accepts
template <typename IDX>
int apm_banded(const DevIndex<IDX> &ix, const DevQueries &qs,
               const uint32_t *dk, uint32_t maxk, ApmRegions &rg,
               Timer &tband, hipStream_t stream, DevBuf &matches,
               uint64_t *nhits, uint64_t *naligned)
{
  const uint64_t nregions = rg.n;
  DevBuf rcount, roffsets, hitpos, hitregion, cand, keep, dcount;
  uint64_t ncand = 0;
  if (rcount.alloc((nregions + 1) * 8) || roffsets.alloc((nregions + 1) * 8))
  {
    return -100;
  }
  VSA_HIP(hipMemsetAsync(rcount.as<uint64_t>() + nregions, 0, 8, stream));
  k_apm_candidates<true, IDX><<<gridfor(nregions), VSA_BLOCK, 0, stream>>>(
      rg.keys.as<uint64_t>(), rg.pbits, dk, nregions, rg.rq.as<uint32_t>(),
      rg.rfirst.as<uint32_t>(), rcount.as<uint64_t>(),
      roffsets.as<uint64_t>(), nullptr, nullptr);
  VSA_HIP(hipGetLastError());
  if (exclusive_sum(rcount.as<uint64_t>(), roffsets.as<uint64_t>(), nregions,
                    stream, &ncand))
  {
    return -100;
  }
  if (ncand >= 0xFFFFFFFFull)
  {
    VSA_ERROR("approximate search: more than 2^32 start positions");
    return -5;
  }
  if (hitpos.alloc(ncand * sizeof(IDX)) || hitregion.alloc(ncand * 4) ||
      cand.alloc(ncand * sizeof(vsa_match)) || keep.alloc(ncand) ||
      matches.alloc(ncand * sizeof(vsa_match)) || dcount.alloc(8))
  {
    return -100;
  }
  k_apm_candidates<false, IDX><<<gridfor(nregions), VSA_BLOCK, 0, stream>>>(
      rg.keys.as<uint64_t>(), rg.pbits, dk, nregions, rg.rq.as<uint32_t>(),
      rg.rfirst.as<uint32_t>(), rcount.as<uint64_t>(),
      roffsets.as<uint64_t>(), hitpos.as<IDX>(), hitregion.as<uint32_t>());
  VSA_HIP(hipGetLastError());
  tband.start();
  withband(maxk, [&](auto band) {
    k_apm_banded<decltype(band)::value>
        <<<gridfor(ncand), VSA_BLOCK, 0, stream>>>(
            ix.tis, ix.n, qs, dk, ncand, hitpos.as<IDX>(),
            hitregion.as<uint32_t>(), rg.rq.as<uint32_t>(), rg.rlo.as<IDX>(),
            rg.rhi.as<IDX>(), cand.as<vsa_match>(), keep.as<uint8_t>());
  });
  tband.stop();
  *naligned = ncand;
  VSA_HIP(hipGetLastError());
  if (compact_matches(cand.as<vsa_match>(), keep.as<uint8_t>(), ncand,
                      matches.as<vsa_match>(), dcount.as<uint64_t>(), stream))
  {
    return -100;
  }
  VSA_HIP(hipMemcpyAsync(nhits, dcount.p, 8, hipMemcpyDeviceToHost, stream));
  VSA_HIP(hipStreamSynchronize(stream));
  return 0;
}

// does a query hold a special symbol (a wildcard)?
static int apm_anyspecial(const DevQueries &qs, uint64_t nq,
                          hipStream_t stream, uint32_t *any)
{
  DevBuf dflag;
  if (dflag.alloc(4))
  {
    return -100;
  }
  VSA_HIP(hipMemsetAsync(dflag.p, 0, 4, stream));
  k_apm_anyspecial<<<gridfor(nq), VSA_BLOCK, 0, stream>>>(
      qs, nq, dflag.as<uint32_t>());
  VSA_HIP(hipMemcpyAsync(any, dflag.p, 4, hipMemcpyDeviceToHost, stream));
  VSA_HIP(hipStreamSynchronize(stream));
  return 0;
}

template <typename IDX>
int run_approx(const vsa_index *index, const vsa_queries *queries,
               bool doedist, const ApmPlan &plan, vsa_result *res)
{
  hipStream_t stream = index->stream;
  vsa_dev_set_stream(stream);
  Timer tall(stream), tsearch(stream), tband(stream);
  const DevIndex<IDX> ix = index->view<IDX>();
  const DevQueries qs = devqueries(queries);
  const uint64_t nq = plan.qlimit, npieces = plan.npieces(nq);
  ApmPieces pc;
  ApmRegions rg;
  DevBuf left, count, offsets, matches;
  uint64_t total = 0, nhits = 0;
  uint32_t special = 0;
  int rc;

  res->stats.searches = npieces;
  if (nq == 0 || npieces == 0)
  {
    return 0;
  }
  if ((rc = apm_positionbits<IDX>(index, queries, 0xFFFFFFFFull,
                                  &rg.pbits)) != 0 ||
      (rc = apm_anyspecial(qs, nq, stream, &special)) != 0)
  {
    return rc;
  }
  if (!doedist && special != 0)
  {
    VSA_ERROR("Hamming distance search with special symbols in a query is "
              "not covered by the GPU engine");
    return VSA_NOT_COVERED;
  }
  // edit distance: start positions by banded alignment unless a query holds
  // a wildcard (the region scan compares raw bytes for m > 32, so that the
  // two ways could then differ) or a threshold exceeds the band
  const uint32_t maxk = plan.maxk(nq);
  const char *nofast = getenv("VSA_APM_SCAN");
  const bool banded = doedist && special == 0 && maxk <= VSA_APM_BANDK &&
                      !(nofast != nullptr && strcmp(nofast, "1") == 0);
  if (pc.alloc(nq, npieces) || left.alloc(npieces * 8) ||
      count.alloc((npieces + 1) * 8) || offsets.alloc((npieces + 1) * 8))
  {
    return -100;
  }
  tall.start();
  if ((rc = apm_pieces(plan, qs, nq, stream, pc)) != 0 ||
      (rc = apm_searchpieces<IDX>(ix, qs, pc, npieces, tsearch, stream,
                                  left.as<uint64_t>(),
                                  count.as<uint64_t>())) != 0)
  {
    return rc;
  }
  if (exclusive_sum(count.as<uint64_t>(), offsets.as<uint64_t>(), npieces,
                    stream, &total))
  {
    return -100;
  }
  res->stats.candidates = total;
  if (total >= 0xFFFFFFFFull)
  {
    VSA_ERROR("approximate search: more than 2^32 piece hits");
    return -5;
  }
  if (total > 0)
  {
    const ApmHits hits = {left.as<uint64_t>(), offsets.as<uint64_t>(),
                          pc.query.as<uint32_t>(), pc.poffset.as<uint32_t>(),
                          npieces, total};
    if ((rc = apm_regions<IDX>(ix, qs, nq, hits, pc.k.as<uint32_t>(), doedist,
                               pc.piecebase.as<uint64_t>(), stream, rg)) != 0)
    {
      return rc;
    }
    rc = banded ? apm_banded<IDX>(ix, qs, pc.k.as<uint32_t>(), maxk, rg, tband,
                                  stream, matches, &nhits,
                                  &res->stats.kernel_searches)
                : apm_verify<IDX>(ix.tis, qs, pc.k.as<uint32_t>(),
                                  (int) ((plan.maxm + 63) / 64), doedist, rg,
                                  stream, matches, &nhits);
    if (rc != 0)
    {
      return rc;
    }
  }
  rc = finish(res, matches, nhits, tall, tsearch, stream);
  res->stats.first_kernel_ms = tband.ms(); // the banded alignment (K <= 3)
  return rc;
}
