// MUM work reduction: first pass and work plan -- kernels; included by
// esa_search.hip (one translation unit: the kernels share the device functions
// of esa_device.hpp and the host pipelines of esa_search.hip launch them).
//
// The idea everything here rests on: if the query suffix at offset j matches
// the text up to the END of the query, no offset j' > j of that query can
// produce a MUM candidate: its longest match is the rest of the query as well,
// and if that match is unique in the index it is the one at (position + j' -
// j), whose left neighbour is the matched query symbol, so the test of
// leftrightmaximaluniquematch / PROCESSSUFFIX (Vmengine/fquery.c:54-81,
// 297-386) rejects it; if it is not unique it is rejected as well.  (The
// reference's own algorithm 2 exploits the same suffix-link structure,
// kurtz/matchsub.c:400-491.)  Round 1 began with an "anchor pass" from the
// last offset of every read (profiles/r01); the first pass from offset 0 and
// the work plan replaced it.


// ---- MUM work plan -------------------------------------------------------
//
// e(j) = j + (length of the longest match of the query suffix at offset j)
// never decreases with j, and an offset whose e equals that of the offset in
// front of it cannot be a MUM candidate: its longest match is the one of its
// predecessor moved by one symbol, so it is either not unique or not left
// maximal (leftrightmaximaluniquematch / PROCESSSUFFIX, fquery.c:54-81,
// 297-386; the reference's default algorithm 2 rides the same suffix links,
// matchsub.c:400-491).  So after the suffix at offset j has been located,
// with E = e(j): if the suffix at jp = E + 1 - l (the last one whose first l
// symbols end at E) also stops at E, every offset in (j, jp] stops at E and
// is dead; the offsets (jp, E] have to be searched, and E + 1 starts afresh.
// A read with one substitution at x costs 1 + l searches instead of x + 2.
//
// A plan is at most VSA_PLAN_RANGES ranges of offsets per query, 16 bits
// each for first offset and length.

#define VSA_PLAN_RANGES 4
#define VSA_PLAN_ROUNDS 6
#define VSA_PLAN_UNKNOWN 0xFFFFFFFFu

#ifndef VSA_PLAN_WAVES
#define VSA_PLAN_WAVES 1
#endif
#ifndef VSA_FIRST_WAVES
#define VSA_FIRST_WAVES 1
#endif
struct PlanRanges
{
  uint32_t r[VSA_PLAN_RANGES]; // first | length << 16
};

__device__ __forceinline__ void plan_add(PlanRanges &pr, uint32_t &nr,
                                         uint32_t first, uint32_t last)
{
  // [first, last], behind everything added so far
  if (first > last)
  {
    return;
  }
  if (nr > 0)
  {
    const uint32_t pf = pr.r[nr - 1] & 0xFFFFu, pl = pr.r[nr - 1] >> 16;
    if (pf + pl == first || nr == VSA_PLAN_RANGES)
    {
      // contiguous, or no slot left: extend the last range up to here
      // (searching a dead offset is harmless, it reports nothing)
      pr.r[nr - 1] = pf | ((last - pf + 1) << 16);
      return;
    }
  }
  pr.r[nr++] = first | ((last - first + 1) << 16);
}

// one work-item per listed query (those with many offsets to search).
// (Round 2 tried the query packed into registers once per work-item
// (vsa_pq_load + vsa_locate_deep<.., PQ>): 439 us instead of 395 -- most
// locates of the plan stop within their first 32 symbols, and the seven loads
// up front cost more than they save.  Not kept.)
// EMIT (deep tables): an offset the plan locates itself (search A of a round:
// the fresh start behind a mismatch, usually a match to the end of the read --
// the expensive kind) is not handed to the search kernel to be located again;
// its candidate, if it is one, is written here, into cursor regions of the
// plan's own (region = workgroup & shardmask, room for every search A of the
// workgroups that share it: no overflow), in the search kernel's form.
struct PlanEmit
{
  const uint64_t *base; // work-item number of (q, 0), or nullptr: q * perquery
  uint32_t perquery;
  vsa_match *out;
  uint64_t *outkey;
  uint64_t shardcap;
  uint32_t shardmask;
  unsigned long long *cursors;
  uint32_t packbits, valbits;
};

// ROWS (DEEP, packed batches): the read comes into registers once, every
// locate of the plan looks at it there.
template <typename IDX, bool DEEP, bool EMIT = false, bool ROWS = false>
__global__ void __launch_bounds__(VSA_BLOCK, VSA_PLAN_WAVES)
k_mum_plan(const DevIndex<IDX> ix, const DevQueries qs,
           const uint32_t *__restrict__ list,
           const uint64_t *__restrict__ nlistword, uint32_t searchlength,
           const uint32_t *__restrict__ firste, uint32_t *__restrict__ count,
           PlanRanges *__restrict__ plan, const PlanEmit em = PlanEmit())
{
  // The length of the list is a number the device knows (low half of
  // *nlistword, written by the scan in front of k_wanted_fill) and the host
  // does not wait for: the launch covers all reads, the workgroups behind the
  // end of the list leave at once.
  const uint64_t nlist = *nlistword & 0xFFFFFFFFull;
  if (vsa_bid() * VSA_BLOCK >= nlist)
  {
    return;
  }
  const uint64_t t = vsa_bid() * VSA_BLOCK + threadIdx.x;
  bool busy = t < nlist;
  uint64_t q = 0;
  uint32_t need = 0, j = 0, nr = 0;
  // offset 0 has been located by k_mum_first: its e is known, and it is
  // not searched again
  uint32_t e0 = VSA_PLAN_UNKNOWN;
  uint32_t qlen = qs.uniformlen;
  const uint8_t *qstart = qs.symbols;
  PlanRanges pr;

#pragma unroll
  for (int i = 0; i < VSA_PLAN_RANGES; i++)
  {
    pr.r[i] = 0;
  }
  RowQuery rq;
  QSrc src;
  bool flagged = false; // ROWS: a read with a special symbol (byte path)
  if constexpr (ROWS)
  {
    rq.row = qs.rows;
    rq.valid = 0;
    src.row = qs.rows;
    src.bytes = nullptr;
    src.pos = src.m = 0;
  }
  if (busy)
  {
    q = list[t];
    need = count[q];
    if constexpr (ROWS)
    {
      flagged = vsa_row_of(qs, q, qlen, rq, src);
    } else
    {
      qstart = qs.dense ? qs.symbols + q * qs.uniformlen
                        : qs.symbols + qs.start[q];
      if (!qs.dense)
      {
        qlen = (uint32_t) qs.length[q];
      }
    }
    if (firste != nullptr)
    {
      e0 = firste[q];
    }
  }
  for (int round = 0; round < VSA_PLAN_ROUNDS && __any(busy); round++)
  {
    // A: the suffix at offset j
    uint32_t maxlcp = 0, maxlcp2 = 0;
    uint64_t witness = 0;
    bool have = false, have2 = false;
    const bool known = round == 0 && e0 != VSA_PLAN_UNKNOWN;
    // EMIT: this lane answers offset j itself if the range behind it can open
    // a slot of its own (with none left, plan_add stretches the last range
    // over the gap, and the search kernel would answer j a second time)
    const bool answers = DEEP && EMIT && nr < VSA_PLAN_RANGES;
    if (busy && !known && need - j <= 2)
    {
      plan_add(pr, nr, j, need - 1); // nothing to gain any more
      busy = false;
    }
    if constexpr (DEEP)
    {
      DeepHit hit;
      // (a fresh start usually matches far: two text pieces per round trip)
      int st;
      if constexpr (ROWS)
      {
        // (windows of the row; a read with a special symbol -- rare -- takes
        // the reference walk on its bytes, the path of every lane the deep
        // locate hands back)
        st = vsa_locate_deep<2, true>(ix, busy && !known && !flagged, src + j,
                                      qlen - j, maxlcp, witness, hit,
                                      EMIT ? searchlength : 0xFFFFFFFFu,
                                      0x100u, &rq, j);
        if (busy && !known && flagged)
        {
          st = VSA_LOC_SLOW;
        }
      } else
      {
        st = vsa_locate_deep<2>(ix, busy && !known, qstart + j, qlen - j,
                                maxlcp, witness, hit,
                                EMIT ? searchlength : 0xFFFFFFFFu);
      }
      if (st == VSA_LOC_SLOW)
      {
        if constexpr (ROWS)
        {
          have = vsa_locate_reference(ix, src + j, qlen - j, maxlcp, witness);
        } else
        {
          have = vsa_locate_reference(ix, qstart + j, qlen - j, maxlcp,
                                      witness);
        }
      } else
      {
        have = st == VSA_LOC_FOUND;
      }
      if constexpr (EMIT)
      {
        // the candidate test of k_query_search_planned for work-item (q, j)
        // (j >= 1: offset 0 belongs to the first pass)
        const bool fast = st != VSA_LOC_SLOW && have && maxlcp < 255;
        uint32_t c = 0;
        uint8_t leftchar = (uint8_t) VSA_SEPARATOR;
        if (answers && busy && !known && have && maxlcp >= searchlength)
        {
          if (j > 0) // offset 0: the start of the query is left maximal
          {
            if constexpr (ROWS)
            {
              leftchar = vsa_qsym(src, j - 1);
            } else
            {
              leftchar = qstart[j - 1];
            }
          }
          if (fast)
          {
            const uint32_t lcpw = (uint32_t) (hit.ew >> 32) & 0xFFu;
            const bool unique =
                (witness == 0 || lcpw < maxlcp) &&
                (witness + 1 > ix.n - 1 || hit.lcpnext < maxlcp);
            c = (unique &&
                 (VSA_ISSPECIAL(leftchar) || leftchar != hit.leftsym))
                    ? 1u
                    : 0u;
          } else
          {
            c = (vsa_mum_candidate<IDX, true>(ix, maxlcp, witness) &&
                 vsa_leftmaximal(ix, vsa_sufstart<IDX, true>(ix, witness),
                                 leftchar))
                    ? 1u
                    : 0u;
          }
        }
        const uint32_t shard = (uint32_t) vsa_bid() & em.shardmask;
        const uint64_t inshard = vsa_wave_reserve01(
            em.cursors + (uint64_t) shard * VSA_CURSOR_STRIDE, c != 0);
        if (c != 0 && inshard < em.shardcap)
        {
          const uint64_t dbstart = fast ? vsa_entrystart(ix, hit.ew, witness)
                                        : vsa_sufstart<IDX, true>(ix, witness);
          const uint64_t t0 =
              (em.base != nullptr) ? em.base[q] : q * em.perquery;
          vsa_write_candidate(qs, em.out, em.outkey,
                              (uint64_t) shard * em.shardcap + inshard, q, j,
                              t0 + j, dbstart, maxlcp, em.packbits,
                              em.valbits);
        }
      }
    } else
    {
      if (busy && !known)
      {
        have = vsa_locate_reference(ix, qstart + j, qlen - j, maxlcp, witness);
      }
    }
    if (known)
    {
      have = true;
      maxlcp = e0;
    }
    uint32_t E = 0, jp = 0;
    bool probe = false;
    if (busy)
    {
      if (!known && !answers)
      {
        plan_add(pr, nr, j, j); // (else: answered above)
      }
      if (!have)
      {
        // fewer than prefixlength symbols match: no exact E; the offsets
        // up to there are searched, the next round starts behind them
        const uint32_t last = (j + ix.pl - 1 < need - 1) ? j + ix.pl - 1
                                                         : need - 1;
        plan_add(pr, nr, j + 1, last);
        j = last + 1;
        busy = j < need;
      } else
      {
        E = j + maxlcp;
        if (E >= qlen)
        {
          busy = false; // matches to the end: every later offset is dead
        } else
        {
          probe = E + 1 >= searchlength + j + 3 &&
                  E + 1 - searchlength < need;
          jp = probe ? E + 1 - searchlength : 0;
        }
      }
    }
    // B: the probe at jp
    const bool doprobe = busy && have && probe;
    if constexpr (DEEP)
    {
      DeepHit hit;
      int st;
      if constexpr (ROWS)
      {
        st = vsa_locate_deep<1, true>(ix, doprobe && !flagged, src + jp,
                                      qlen - jp, maxlcp2, witness, hit,
                                      0xFFFFFFFFu, 0x100u, &rq, jp);
        if (doprobe && flagged)
        {
          st = VSA_LOC_SLOW;
        }
      } else
      {
        st = vsa_locate_deep(ix, doprobe, qstart + jp, qlen - jp, maxlcp2,
                             witness, hit);
      }
      if (st == VSA_LOC_SLOW)
      {
        if constexpr (ROWS)
        {
          have2 = vsa_locate_reference(ix, src + jp, qlen - jp, maxlcp2,
                                       witness);
        } else
        {
          have2 = vsa_locate_reference(ix, qstart + jp, qlen - jp, maxlcp2,
                                       witness);
        }
      } else
      {
        have2 = st == VSA_LOC_FOUND;
      }
    } else
    {
      if (doprobe)
      {
        have2 = vsa_locate_reference(ix, qstart + jp, qlen - jp, maxlcp2,
                                     witness);
      }
    }
    if (busy && have)
    {
      const bool dead = doprobe && have2 && jp + maxlcp2 == E;
      const uint32_t first = dead ? jp + 1 : j + 1;
      const uint32_t last = (E < need - 1) ? E : need - 1;
      plan_add(pr, nr, first, last);
      j = E + 1;
      busy = j < need;
    }
  }
  if (t < nlist)
  {
    if (busy)
    {
      plan_add(pr, nr, j, need - 1); // out of rounds: search the rest
    }
    uint32_t total = 0;
#pragma unroll
    for (int i = 0; i < VSA_PLAN_RANGES; i++)
    {
      total += pr.r[i] >> 16;
    }
    plan[q] = pr;
    count[q] = total;
  }
}


#include "mum_walk.inc"

// what a workgroup of k_query_search_planned did: the locates it made
// (stats.kernel_searches) and the offsets of its plans (the planned term of
// stats.searches, which counts the work the plan asked for and does not
// depend on how the search kernel goes through it)
struct PlannedWork
{
  unsigned long long locates, offsets;
};
struct PlannedWorkPlus
{
  __host__ __device__ PlannedWork operator()(const PlannedWork &a,
                                             const PlannedWork &b) const
  {
    return PlannedWork{a.locates + b.locates, a.offsets + b.offsets};
  }
};

// 8 wavefronts per SIMD (64 VGPRs, no scratch; the compiler takes 75 when
// left alone: 1.50-1.55 against 1.57 ms)
#ifndef VSA_P1_WAVES
#define VSA_P1_WAVES 8
#endif
// The MUM forms carry the walk's state (chunk, offset, read) around the
// locate and, on packed batches, a second copy of the walk for the reads with
// a special symbol: 74 to 76 VGPRs.  Held to 64 they spill 10 to 13 VGPRs to
// scratch (40 to 56 bytes per lane), at 7 wavefronts (72 VGPRs) the packed
// form still spills 20 bytes: 6 wavefronts per SIMD, no scratch.  (The tile
// queue: 66 VGPRs on bytes, 80 on rows, no scratch -- profiles/r16.)
#ifndef VSA_WALK_WAVES
#define VSA_WALK_WAVES 6
#endif
// Reads per lane of a workgroup of the MUM forms.  A quarter of the headline's
// reads has a plan, of one range that is one chunk: with BLK reads per
// workgroup one wavefront of four walked and the others waited for it at the
// barrier (3.70 ms per step against the parent's 2.90, profiles/r13).  Four
// reads per lane fill the workgroup.
#ifndef VSA_WALK_READS
#define VSA_WALK_READS 4
#endif
// K2 in its workgroup tiles, straight from the plans (the MEM plan; the MUM
// forms under VSA_TUNE=32 -- by default they take the tile queue,
// k_mum_walk_tiles below): a workgroup takes BLK consecutive queries, lays their planned offsets out in LDS (a scan of the
// counts, the ranges of every plan) and walks that list BLK work-items at a
// time -- no expanded work list in memory (8 bytes per work-item written and
// read back in round 1), no scan over all queries, no host round trip before
// the launch.  Per work-item exactly what k_query_search<IDX, MUM, DEEP> does
// (same device functions, same output form, same sort key).
// blocksum[workgroup] = the locates it made and the offsets its plans hold
// (PlannedWork).  DEEP = false: indexes without the deep tables (other
// alphabets, VSA_NO_ESA8): the reference walk per item.
//
// The walk (MUM = true).  A work-item is a chunk of a plan range, at most
// 1 << chunkshift offsets, walked by one lane from its last offset down.
// e(j) never decreases with j (above), so once offset h is located every
// j < h has a longest match of at most e(h) - j, and a candidate needs
// searchlength symbols: the offsets j with e(h) - searchlength < j < h are no
// candidates and are not located.  The lane goes on at
// min(h - 1, h + U - searchlength), U an UPPER bound of the longest match at h:
//   VSA_LOC_FOUND              maxlcp (exact), or no bound at all where the
//                              locate was cut short (hit.notleftmax: maxlcp
//                              is a lower bound, only h itself is done)
//   VSA_LOC_NONE               D - 1: nothing shares D symbols
//   the reference walk         maxlcp (exact), or prefixlength - 1 without a
//                              bucket
// A random 20-mer matches log4 n symbols, 15 to 17 in a 3 Gbp text: a locate
// disposes of about five offsets of a range behind a substitution.  Every
// located offset takes the candidate test and the output form of the
// one-offset-per-work-item kernel, so the lists do not change; a chunk makes at
// most as many locates as it has offsets.  chunkshift = 0 (VSA_TUNE=16) is
// that kernel: every planned offset located.
// The deep locate wants all lanes of a wavefront: the walk is a loop with a
// wavefront-uniform exit, finished lanes pass active = false.
// ROWS (DEEP, packed batches): a work-item takes its read from the row (two
// 16-byte loads, the neighbouring offsets of a read share them).
// MUM = false (byte batches): the planned offsets of a MEM batch
// (mem_workplan.inc), each through vsa_query_item<MEM>.
template <typename IDX, int BLK, bool DEEP = true, bool ROWS = false,
          bool MUM = true>
__global__ void __launch_bounds__(BLK, MUM ? VSA_WALK_WAVES : VSA_P1_WAVES)
k_query_search_planned(const DevIndex<IDX> ix, const DevQueries qs,
                       const uint64_t *__restrict__ base, uint32_t perquery,
                       const PlanRanges *__restrict__ plan,
                       const uint32_t *__restrict__ plancount,
                       uint32_t searchlength, vsa_match *__restrict__ out,
                       uint64_t *__restrict__ outkey, uint64_t shardcap,
                       uint32_t shardmask,
                       unsigned long long *__restrict__ cursors,
                       uint32_t packbits, uint32_t valbits,
                       PlannedWork *__restrict__ blocksum,
                       uint32_t chunkshift = 0)
{
  // reads per lane and per workgroup (see VSA_WALK_READS)
  constexpr int RPT = MUM ? VSA_WALK_READS : 1, RPB = BLK * RPT;
  __shared__ uint32_t rel[RPB + 1];
  __shared__ PlanRanges pr[RPB];
  // (the MUM forms only)
  __shared__ uint64_t lanesum[MUM ? BLK + 1 : 1];
  __shared__ uint32_t wavelocates[MUM ? BLK / 64 : 1];
  const uint64_t q0 = vsa_bid() * RPB;
  const uint32_t tid = threadIdx.x;
  // (the MEM plan: one offset per work-item)
  const uint32_t cshift = MUM ? chunkshift : 0, chunk = 1u << cshift;
  if constexpr (!MUM)
  {
    const bool in = q0 + tid < qs.nq;
    const uint32_t mine = in ? plancount[q0 + tid] : 0;
    if (in)
    {
      pr[tid] = plan[q0 + tid];
    }
    // exclusive scan of the counts
    rel[tid + 1] = mine;
    if (tid == 0)
    {
      rel[0] = 0;
    }
    __syncthreads();
    for (uint32_t d = 1; d < BLK; d <<= 1)
    {
      const uint32_t v = (tid + 1 > d) ? rel[tid + 1 - d] : 0;
      __syncthreads();
      rel[tid + 1] += v;
      __syncthreads();
    }
  } else
  {
    // the counts of RPT consecutive reads per lane, chunks instead of
    // offsets, summed up as they come; the planned offsets ride along in the
    // upper half of the lanes' sums (a workgroup plans fewer than 2^32, no
    // carry) -- summed in registers and by shuffles they cost the packed form
    // 24 bytes of scratch per lane
    uint32_t mine[RPT], sum = 0, offsets = 0;
#pragma unroll
    for (int k = 0; k < RPT; k++)
    {
      const uint64_t q = q0 + tid * RPT + k;
      uint32_t c = q < qs.nq ? plancount[q] : 0;
      offsets += c;
      if (q < qs.nq)
      {
        const PlanRanges p = plan[q];
        pr[tid * RPT + k] = p;
        if (c > 0)
        {
          c = 0;
#pragma unroll
          for (int g = 0; g < VSA_PLAN_RANGES; g++)
          {
            c += ((p.r[g] >> 16) + chunk - 1) >> cshift;
          }
        }
      }
      sum += c;
      mine[k] = sum;
    }
    // exclusive scan of the lanes' sums
    lanesum[tid + 1] = sum | ((uint64_t) offsets << 32);
    if (tid == 0)
    {
      lanesum[0] = 0;
      rel[0] = 0;
    }
    __syncthreads();
    for (uint32_t d = 1; d < BLK; d <<= 1)
    {
      const uint64_t v = (tid + 1 > d) ? lanesum[tid + 1 - d] : 0;
      __syncthreads();
      lanesum[tid + 1] += v;
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < RPT; k++)
    {
      rel[tid * RPT + k + 1] = (uint32_t) lanesum[tid] + mine[k];
    }
    __syncthreads();
  }
  const uint32_t total = rel[RPB];
  if (tid == 0)
  {
    // (MUM: the locates follow at the end)
    if constexpr (MUM)
    {
      blocksum[vsa_bid()].offsets = lanesum[BLK] >> 32;
    } else
    {
      blocksum[vsa_bid()] = PlannedWork{total, total};
    }
  }
  const uint32_t shard = vsa_bid() & shardmask;
  uint32_t locates = 0; // of this lane
  for (uint32_t i0 = 0; i0 < total; i0 += BLK)
  {
    const uint32_t i = i0 + tid;
    bool active = i < total;
    // MUM: the chunk is [first, off], off comes down as the walk goes
    uint32_t off = 0, first = 0, qlen = qs.uniformlen;
    uint64_t q = 0, t0 = 0;
    const uint8_t *qstart = qs.symbols;
    if (active)
    {
      // the query whose stretch holds item i: last k with rel[k] <= i
      uint32_t lo = 0, hi = RPB;
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
      // its chunk: the r-th of the read's ranges, each cut from its first
      // offset on
      uint32_t r = i - rel[lo];
#pragma unroll
      for (int k = 0; k < VSA_PLAN_RANGES; k++)
      {
        const uint32_t rf = pr[lo].r[k] & 0xFFFFu, len = pr[lo].r[k] >> 16,
                       nchunks = (len + chunk - 1) >> cshift;
        if (r < nchunks)
        {
          const uint32_t at = r << cshift,
                         n = len - at < chunk ? len - at : chunk;
          first = rf + at;
          off = first + n - 1;
          r = 0xFFFFFFFFu; // found: no later range takes it
        } else if (r != 0xFFFFFFFFu)
        {
          r -= nchunks;
        }
      }
      q = q0 + lo;
      if constexpr (!MUM)
      {
        t0 = (base != nullptr) ? base[q] : q * perquery;
      }
      if constexpr (MUM && !ROWS)
      {
        if (qs.dense)
        {
          qstart = qs.symbols + q * qs.uniformlen;
        } else
        {
          qstart = qs.symbols + qs.start[q];
          qlen = (uint32_t) qs.length[q];
        }
      }
    }
    if constexpr (!MUM)
    {
      // (vsa_query_item finds the symbols itself)
      vsa_query_item<IDX, false, DEEP>(ix, qs, active, q, off, t0 + off,
                                       searchlength, out, outkey, shardcap,
                                       shard, cursors, 0, 0);
      continue;
    }
    if constexpr (DEEP && ROWS)
    {
      // windows of the row; a read with a special symbol (rare) is walked on
      // its bytes behind the others, as the byte form walks it
      RowQuery rq;
      QSrc src;
      bool flagged = false;
      rq.row = qs.rows;
      rq.valid = 0;
      src.row = qs.rows;
      src.bytes = nullptr;
      src.pos = src.m = 0;
      if (active)
      {
        flagged = vsa_row_of(qs, q, qs.uniformlen, rq, src);
      }
      locates += vsa_walk_chunk<IDX, true, true>(
          ix, qs, active && !flagged, src, &rq, qlen, first, off, q, base,
          perquery, searchlength, out, outkey, shardcap, shard, cursors,
          packbits, valbits);
      if (__any(active && flagged))
      {
        locates += vsa_walk_chunk<IDX, true, false>(
            ix, qs, active && flagged, src, nullptr, qlen, first, off, q, base,
            perquery, searchlength, out, outkey, shardcap, shard, cursors,
            packbits, valbits);
      }
    } else
    {
      locates += vsa_walk_chunk<IDX, DEEP, false>(
          ix, qs, active, qstart, nullptr, qlen, first, off, q, base, perquery,
          searchlength, out, outkey, shardcap, shard, cursors, packbits,
          valbits);
    }
  }
  if constexpr (MUM)
  {
    // blocksum[workgroup] = the locates of its lanes, its planned offsets
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
    {
      locates += __shfl_xor(locates, d, 64);
    }
    if ((tid & 63u) == 0)
    {
      wavelocates[tid >> 6] = locates;
    }
    __syncthreads();
    if (tid == 0)
    {
      uint32_t s = 0;
#pragma unroll
      for (int w = 0; w < BLK / 64; w++)
      {
        s += wavelocates[w];
      }
      blocksum[vsa_bid()].locates = s;
    }
  }
}

// ---- the tile queue ------------------------------------------------------
//
// K2 for a planned MUM batch as every call runs it (VSA_TUNE=32 takes the MUM
// forms back to k_query_search_planned above): the same chunks through the
// same step, vsa_walk_step, handed out differently.  Above, a lane keeps one
// chunk per pass and a workgroup keeps its slot until its slowest wavefront is
// done; a chunk takes 1 to 8 dependent locates on the headline, so the
// wavefronts went round with about 0.6 of their lanes busy.  Here a wavefront
// works on its own: it takes tiles of 64 consecutive entries of the list of
// the reads that have a plan (the list k_mum_plan works from, its length read
// on the device) from one counter in global memory, and in front of EVERY
// step its free lanes take the next chunks of the tile, the next tile when
// that one is used up.  Nothing waits for another wavefront: no
// __syncthreads(), the launch is as large as the device holds (any other size
// is as right), and the reads without a plan are never looked at.
//
// A tile lies in the wavefront's own slice of LDS: the reads, their ranges and
// the exclusive prefix of their chunk counts.  Chunk i of the tile belongs to
// the last read k with pre[k] <= i and is its (i - pre[k])-th chunk, ranges
// cut from their first offset on as above.  Head and tail of the tile are
// wavefront-uniform.
struct WalkTile
{
  PlanRanges pr[64];
  uint32_t q[64];
  uint32_t pre[65];
};
// chunks of reads of a packed batch that have a special symbol, set aside for
// the byte form of the step (read, first | off << 16): filled up to 64 + 63
#define VSA_WALK_ASIDE 128
struct WalkAside
{
  uint32_t q[VSA_WALK_ASIDE], r[VSA_WALK_ASIDE];
};

// what one lane wrote into the wavefront's slice before, every lane of it sees
// behind this (LDS operations of a wavefront run in order: the compiler has to
// keep them so, nothing has to be waited for)
__device__ __forceinline__ void vsa_wave_lds_fence()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the lanes of `mask` in front of this one
__device__ __forceinline__ uint32_t vsa_rank_in(uint64_t mask)
{
  return __builtin_amdgcn_mbcnt_hi(
      (uint32_t) (mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) mask, 0u));
}

// the r-th chunk of a plan: [first, off]
__device__ __forceinline__ void vsa_plan_chunk(const PlanRanges &p, uint32_t r,
                                               uint32_t cshift,
                                               uint32_t &first, uint32_t &off)
{
  const uint32_t chunk = 1u << cshift;
#pragma unroll
  for (int k = 0; k < VSA_PLAN_RANGES; k++)
  {
    const uint32_t rf = p.r[k] & 0xFFFFu, len = p.r[k] >> 16,
                   nchunks = (len + chunk - 1) >> cshift;
    if (r < nchunks)
    {
      const uint32_t at = r << cshift, n = len - at < chunk ? len - at : chunk;
      first = rf + at;
      off = first + n - 1;
      r = 0xFFFFFFFFu; // found: no later range takes it
    } else if (r != 0xFFFFFFFFu)
    {
      r -= nchunks;
    }
  }
}

// blocksum[4 * workgroup + wavefront] = the locates the wavefront made and the
// planned offsets of the tiles it took.  tilecounter: zero at the launch.
// ROWS: the chunks of a read with a special symbol go to the aside list and
// are walked on the read's bytes, 64 at a time, when no lane has a chunk of
// the other kind (with 64 of them waiting nothing new is handed out), so that
// the two forms of the step never run with each other's state alive.
template <typename IDX, bool DEEP = true, bool ROWS = false>
__global__ void __launch_bounds__(256, VSA_WALK_WAVES)
k_mum_walk_tiles(const DevIndex<IDX> ix, const DevQueries qs,
                 const uint64_t *__restrict__ base, uint32_t perquery,
                 const PlanRanges *__restrict__ plan,
                 const uint32_t *__restrict__ plancount,
                 const uint32_t *__restrict__ list,
                 const uint64_t *__restrict__ nlistword,
                 unsigned long long *__restrict__ tilecounter,
                 uint32_t searchlength, vsa_match *__restrict__ out,
                 uint64_t *__restrict__ outkey, uint64_t shardcap,
                 uint32_t shardmask, unsigned long long *__restrict__ cursors,
                 uint32_t packbits, uint32_t valbits,
                 PlannedWork *__restrict__ blocksum, uint32_t chunkshift)
{
  __shared__ WalkTile tiles[4];
  __shared__ WalkAside asides[ROWS ? 4 : 1];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  WalkTile &tile = tiles[wave];
  WalkAside &aside = asides[ROWS ? wave : 0];
  const uint64_t nlist = *nlistword & 0xFFFFFFFFull;
  const uint32_t shard = vsa_bid() & shardmask;
  // of the wavefront: the chunks of its tile are [0, tail), [0, head) are
  // handed out; the counter has run out; chunks set aside
  uint32_t head = 0, tail = 0, naside = 0;
  bool exhausted = false;
  // of the lane: its chunk [first, off] of read q, off comes down
  bool active = false;
  uint32_t off = 0, first = 0, q = 0, qlen = qs.uniformlen;
  uint32_t locates = 0, offsets = 0;
  const uint8_t *qstart = qs.symbols;
  for (;;)
  {
    // hand-out: all lanes are here together
    uint64_t freemask = __ballot(!active);
    while (freemask != 0 && !(ROWS && naside >= 64))
    {
      if (head == tail)
      {
        if (exhausted)
        {
          break;
        }
        // the next tile
        unsigned long long mine = 0;
        if (lane == 0)
        {
          mine = atomicAdd(tilecounter, 1ull);
        }
        const uint64_t t0 =
            ((uint64_t) __builtin_amdgcn_readfirstlane((uint32_t) (mine >> 32))
             << 32) |
            __builtin_amdgcn_readfirstlane((uint32_t) mine);
        if (t0 * 64 >= nlist)
        {
          exhausted = true;
          break;
        }
        const uint64_t t = t0 * 64 + lane;
        uint32_t tq = 0, nch = 0;
        PlanRanges p;
#pragma unroll
        for (int g = 0; g < VSA_PLAN_RANGES; g++)
        {
          p.r[g] = 0;
        }
        if (t < nlist)
        {
          tq = list[t];
          const uint32_t c = plancount[tq];
          p = plan[tq];
          offsets += c;
          if (c > 0)
          {
#pragma unroll
            for (int g = 0; g < VSA_PLAN_RANGES; g++)
            {
              nch += ((p.r[g] >> 16) + (1u << chunkshift) - 1) >> chunkshift;
            }
          }
        }
        const uint32_t incl = vsa_wave_inclusive_sum(nch);
        vsa_wave_lds_fence(); // (the last tile has been read)
        tile.q[lane] = tq;
        tile.pr[lane] = p;
        tile.pre[lane + 1] = incl;
        if (lane == 0)
        {
          tile.pre[0] = 0;
        }
        vsa_wave_lds_fence();
        head = 0;
        tail = __builtin_amdgcn_readlane(incl, 63);
        continue;
      }
      // the free lanes take chunks [head, head + take) by their rank
      const uint32_t nfree = (uint32_t) __popcll(freemask),
                     take = nfree < tail - head ? nfree : tail - head,
                     rank = vsa_rank_in(freemask);
      const bool took = !active && rank < take;
      bool flagged = false;
      if (took)
      {
        const uint32_t i = head + rank;
        // last k with pre[k] <= i
        uint32_t lo = 0;
#pragma unroll
        for (uint32_t d = 32; d >= 1; d >>= 1)
        {
          if (tile.pre[lo + d] <= i)
          {
            lo += d;
          }
        }
        q = tile.q[lo];
        vsa_plan_chunk(tile.pr[lo], i - tile.pre[lo], chunkshift, first, off);
        if constexpr (ROWS)
        {
          RowQuery rq;
          QSrc src;
          flagged = vsa_row_of(qs, q, qs.uniformlen, rq, src);
        } else
        {
          if (qs.dense)
          {
            qstart = qs.symbols + (uint64_t) q * qs.uniformlen;
          } else
          {
            qstart = qs.symbols + qs.start[q];
            qlen = (uint32_t) qs.length[q];
          }
        }
        active = !flagged;
      }
      head += take;
      if constexpr (ROWS)
      {
        const uint64_t fmask = __ballot(flagged);
        if (flagged)
        {
          const uint32_t at = naside + vsa_rank_in(fmask);
          aside.q[at] = q;
          aside.r[at] = first | (off << 16);
        }
        naside += (uint32_t) __popcll(fmask);
      }
      freemask = __ballot(!active);
    }
    if (!__any(active))
    {
      if constexpr (ROWS)
      {
        if (naside > 0)
        {
          // the chunks set aside, on their reads' bytes
          vsa_wave_lds_fence();
          for (uint32_t a0 = 0; a0 < naside; a0 += 64)
          {
            const bool mine = a0 + lane < naside;
            uint32_t aq = 0, afirst = 0, aoff = 0;
            RowQuery arq;
            QSrc src;
            arq.row = qs.rows;
            arq.valid = 0;
            src.row = qs.rows;
            src.bytes = nullptr;
            src.pos = src.m = 0;
            if (mine)
            {
              aq = aside.q[a0 + lane];
              afirst = aside.r[a0 + lane] & 0xFFFFu;
              aoff = aside.r[a0 + lane] >> 16;
              (void) vsa_row_of(qs, aq, qs.uniformlen, arq, src);
            }
            locates += vsa_walk_chunk<IDX, true, false>(
                ix, qs, mine, src, nullptr, qlen, afirst, aoff, aq, base,
                perquery, searchlength, out, outkey, shardcap, shard, cursors,
                packbits, valbits);
          }
          vsa_wave_lds_fence();
          naside = 0;
          // (no lane had a chunk: nothing of the lanes' own state is carried
          // through the walk above)
          q = first = off = 0;
          continue;
        }
      }
      break; // no chunk left in the tile, no tile left in the list
    }
    if constexpr (DEEP && ROWS)
    {
      // (the row from the number of the read: nothing but q travels round
      // the loop)
      RowQuery rq;
      QSrc src;
      rq.row = qs.rows + (uint64_t) q * qs.roww;
      rq.valid = qlen;
      src.row = rq.row;
      src.bytes = nullptr;
      src.pos = 0;
      src.m = (int32_t) qlen;
      vsa_walk_step<IDX, true, true>(ix, qs, active, src, &rq, qlen, first,
                                     off, q, base, perquery, searchlength, out,
                                     outkey, shardcap, shard, cursors, packbits,
                                     valbits, locates);
    } else
    {
      vsa_walk_step<IDX, DEEP, false>(ix, qs, active, qstart, nullptr, qlen,
                                      first, off, q, base, perquery,
                                      searchlength, out, outkey, shardcap,
                                      shard, cursors, packbits, valbits,
                                      locates);
    }
  }
  uint64_t sum = locates | ((uint64_t) offsets << 32);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1)
  {
    // (a wavefront takes fewer than 2^32 locates: no carry)
    sum += vsa_shfl64(sum, (int) lane ^ d);
  }
  if (lane == 0)
  {
    blocksum[vsa_bid() * 4 + wave] =
        PlannedWork{sum & 0xFFFFFFFFull, sum >> 32};
  }
}

// The first pass of a MUM batch: offset 0 of every query, located with the
// whole query.  A query that matches completely is finished here: e(0) is
// the end of the query, so no later offset can be a candidate (see above),
// and offset 0 is one iff its match is unique -- its left neighbour is the
// start of the query, which PROCESSSUFFIX treats as left maximal
// (fquery.c:54-81).  That is one search for an exact read instead of two
// (last offset + offset 0) and a backward walk.  For the others e(0) goes to
// the work plan.
// PQ (dense batches of reads of m <= 128 symbols, m a multiple of 4; deep
// tables): the workgroup's queries come through LDS with coalesced loads and
// sit packed in registers (vsa_pq_stage); dynamic LDS: VSA_BLOCK * m bytes.
// ROWS (with DEEP and PQ; packed batches, DevQueries::rows): a read is two
// 16-byte loads away from being a PackedQuery -- no LDS, no packing.
// WINDOWS (with ROWS): reads of more than four words (125 symbols and more;
// 150 bp is five) do not fit a PackedQuery: the read stays where it is and
// every look at it is a 16-byte load of its row (RowQuery), as in the plan and
// the search kernel.
template <typename IDX, bool DEEP, bool PQ = false, bool ROWS = false,
          bool WINDOWS = false>
__global__ void __launch_bounds__(VSA_BLOCK, VSA_FIRST_WAVES)
k_mum_first(const DevIndex<IDX> ix, const DevQueries qs, uint32_t perquery,
            uint32_t searchlength, uint32_t *__restrict__ count,
            uint32_t *__restrict__ firste, uint32_t *__restrict__ fmlen,
            uint64_t *__restrict__ fmdb,
            uint64_t *__restrict__ blockcount = nullptr)
{
  // blockcount (MUM batches): per workgroup, reads that want a plan | reads
  // whose offset 0 is a candidate << 32 -- what k_wanted_count counted in a
  // pass of its own over count[] and fmlen[] until round 4
  extern __shared__ uint32_t stagedqueries[];
  __shared__ uint32_t wantwaves[VSA_BLOCK / 64], candwaves[VSA_BLOCK / 64];
  // perquery != 0: every query has the same length (and so many offsets);
  // else ragged: length and offsets per query
  const uint64_t q = vsa_bid() * VSA_BLOCK + threadIdx.x;
  uint32_t qlen = qs.uniformlen, perq = perquery;
  const uint8_t *qptr = qs.symbols;
  uint32_t maxlcp = 0;
  uint64_t witness = 0;
  bool have = false, fast = false;
  DeepHit hit;

  if (!ROWS && q < qs.nq)
  {
    if (qs.dense)
    {
      qptr = qs.symbols + q * qs.uniformlen;
    } else
    {
      qptr = qs.symbols + qs.start[q];
      qlen = (uint32_t) qs.length[q];
      perq = (qlen >= searchlength) ? qlen - searchlength + 1 : 0;
    }
  }
  const bool active = q < qs.nq && perq > 0;
  if constexpr (DEEP && ROWS && WINDOWS)
  {
    RowQuery rq;
    QSrc src;
    bool flagged = false;
    rq.row = qs.rows;
    rq.valid = 0;
    src.row = qs.rows;
    src.bytes = nullptr;
    src.pos = src.m = 0;
    if (q < qs.nq)
    {
      flagged = vsa_row_of(qs, q, qlen, rq, src);
    }
    int st = vsa_locate_deep<3, true>(ix, active && !flagged, src, qlen,
                                      maxlcp, witness, hit, 0xFFFFFFFFu,
                                      0x100u, &rq, 0);
    if (active && flagged)
    {
      st = VSA_LOC_SLOW; // (a read with a special symbol: its bytes)
    }
    if (st == VSA_LOC_SLOW)
    {
      have = vsa_locate_reference(ix, src, qlen, maxlcp, witness);
    } else
    {
      have = st == VSA_LOC_FOUND;
      fast = have && maxlcp < 255;
    }
  } else if constexpr (DEEP && ROWS)
  {
    PackedQuery pq;
    QSrc src;
    pq.w[0] = pq.w[1] = pq.w[2] = pq.w[3] = 0;
    pq.valid = 0;
    src.row = qs.rows;
    src.bytes = nullptr;
    src.pos = src.m = 0;
    if (q < qs.nq)
    {
      vsa_pq_from_row(qs, q, qlen, pq, src);
    }
    const int st = vsa_locate_deep<3, true>(ix, active, src, qlen, maxlcp,
                                            witness, hit, 0xFFFFFFFFu, 0x100u,
                                            &pq);
    if (st == VSA_LOC_SLOW)
    {
      have = vsa_locate_reference(ix, src, qlen, maxlcp, witness);
    } else
    {
      have = st == VSA_LOC_FOUND;
      fast = have && maxlcp < 255;
    }
  } else if constexpr (DEEP)
  {
    // most reads match over their whole length: three 32-symbol pieces of
    // the text per round trip
    int st;
    if constexpr (PQ)
    {
      PackedQuery pq;
      vsa_pq_stage<VSA_BLOCK>(qs, vsa_bid() * VSA_BLOCK, qlen,
                              stagedqueries, pq);
      st = vsa_locate_deep<3, true>(ix, active, qptr, qlen, maxlcp,
                                           witness, hit, 0xFFFFFFFFu, 0x100u,
                                           &pq);
    } else
    {
      st = vsa_locate_deep<3>(ix, active, qptr, qlen, maxlcp, witness, hit);
    }
    if (st == VSA_LOC_SLOW)
    {
      have = vsa_locate_reference(ix, qptr, qlen, maxlcp, witness);
    } else
    {
      have = st == VSA_LOC_FOUND;
      fast = have && maxlcp < 255;
    }
  } else
  {
    if (active)
    {
      have = vsa_locate_reference(ix, qptr, qlen, maxlcp, witness);
    }
  }
  uint32_t len = 0, wanted = 0;
  if (q < qs.nq)
  {
    // (not active: shorter than the search length, skipped,
    // matchsub.c:187-190)
    uint64_t db = 0;
    if (active && have && maxlcp >= searchlength)
    {
      bool unique;
      if (fast)
      {
        const uint32_t lcpw = (uint32_t) (hit.ew >> 32) & 0xFFu;
        unique = (witness == 0 || lcpw < maxlcp) &&
                 (witness + 1 > ix.n - 1 || hit.lcpnext < maxlcp);
        db = vsa_entrystart(ix, hit.ew, witness);
      } else
      {
        unique = vsa_mum_candidate<IDX, DEEP>(ix, maxlcp, witness);
        db = vsa_sufstart<IDX, DEEP>(ix, witness);
      }
      len = unique ? maxlcp : 0;
    }
    wanted = !active ? 0 : ((have && maxlcp >= qlen) ? 0 : perq);
    fmlen[q] = len;
    fmdb[q] = db;
    firste[q] = (active && have) ? maxlcp : VSA_PLAN_UNKNOWN;
    count[q] = wanted;
  }
  if (blockcount != nullptr) // (uniform over the launch)
  {
    const uint64_t wmask = __ballot(wanted > 0), cmask = __ballot(len != 0);
    if ((threadIdx.x & 63) == 0)
    {
      wantwaves[threadIdx.x >> 6] = (uint32_t) __popcll(wmask);
      candwaves[threadIdx.x >> 6] = (uint32_t) __popcll(cmask);
    }
    __syncthreads();
    if (threadIdx.x == 0)
    {
      uint64_t t = 0, f = 0;
#pragma unroll
      for (int w = 0; w < VSA_BLOCK / 64; w++)
      {
        t += wantwaves[w];
        f += candwaves[w];
      }
      blockcount[vsa_bid()] = t | (f << 32);
    }
  }
}

// candidates of the first pass -> behind the matches of the search kernel,
// with the sort key of work-item (query, offset 0).  The place of a candidate:
// the candidates of the workgroups in front (blockoffset, top half: counted
// and scanned together with the list of the reads that want a plan) + those
// in front of it in its own workgroup.  (Round 2 took the places from an
// exclusive scan over all 10 M reads: 58 us and 40 MB more per batch.)
__global__ void __launch_bounds__(VSA_BLOCK)
k_append_first(const uint32_t *__restrict__ fmlen,
               const uint64_t *__restrict__ fmdb,
               const uint64_t *__restrict__ blockoffset, uint64_t nq,
               uint32_t perquery, const uint64_t *__restrict__ qbase,
               uint64_t seqoffset, uint64_t base,
               vsa_match *__restrict__ out, uint64_t *__restrict__ outkey,
               uint32_t packbits, uint32_t valbits)
{
  __shared__ uint32_t waves[VSA_BLOCK / 64];
  const uint64_t q = vsa_bid() * VSA_BLOCK + threadIdx.x;
  const bool have = q < nq && fmlen[q] != 0;
  const uint64_t mask = __ballot(have);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0)
  {
    waves[wave] = (uint32_t) __popcll(mask);
  }
  __syncthreads();
  if (!have)
  {
    return;
  }
  uint64_t slot = (blockoffset[vsa_bid()] >> 32) +
                  (uint32_t) __popcll(mask & ((1ull << lane) - 1));
#pragma unroll
  for (uint32_t w = 0; w < VSA_BLOCK / 64; w++)
  {
    slot += (w < wave) ? waves[w] : 0u;
  }
  if (packbits != 0)
  {
    // the pair form of k_query_search
    outkey[base + slot] =
        (fmdb[q] << packbits) | (((1ull << packbits) - 1) - fmlen[q]);
    if (valbits != 0)
    {
      reinterpret_cast<uint32_t *>(out)[base + slot] =
          (uint32_t) (q << valbits);
    } else
    {
      reinterpret_cast<uint64_t *>(out)[base + slot] =
          (q + seqoffset) << 16;
    }
  } else
  {
    vsa_match m;
    m.length = fmlen[q];
    m.dbstart = fmdb[q];
    m.queryseq = q + seqoffset;
    m.querystart = 0;
    out[base + slot] = m;
    outkey[base + slot] = (qbase != nullptr) ? qbase[q] : q * perquery;
  }
}

struct NonZeroToU32
{
  __device__ uint32_t operator()(uint32_t v) const
  {
    return v != 0 ? 1u : 0u;
  }
};

// The list of the queries that want a plan (count above the threshold), in
// order: counts per workgroup, a scan over the workgroups, the list.  (A
// rocprim::select over the 10 M queries of the headline batch took 105 us;
// these take 50.)
// blockcount[workgroup] = reads that want a plan | first-pass candidates << 32
// (fmlen != nullptr: a read whose offset 0 is a candidate; see k_append_first)
__global__ void __launch_bounds__(VSA_BLOCK)
k_wanted_fill(const uint32_t *__restrict__ count, uint64_t nq,
              uint32_t threshold, const uint64_t *__restrict__ blockoffset,
              uint32_t *__restrict__ list)
{
  __shared__ uint32_t waves[VSA_BLOCK / 64];
  const uint64_t q = vsa_bid() * VSA_BLOCK + threadIdx.x;
  const bool want = q < nq && count[q] > threshold;
  const uint64_t mask = __ballot(want);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0)
  {
    waves[wave] = (uint32_t) __popcll(mask);
  }
  __syncthreads();
  if (want)
  {
    uint32_t at = (uint32_t) blockoffset[vsa_bid()] +
                  (uint32_t) __popcll(mask & ((1ull << lane) - 1));
#pragma unroll
    for (uint32_t w = 0; w < VSA_BLOCK / 64; w++)
    {
      at += (w < wave) ? waves[w] : 0u;
    }
    list[at] = (uint32_t) q;
  }
}

struct PlanWanted
{
  const uint32_t *count;
  uint32_t threshold;
  __device__ bool operator()(uint32_t q) const
  {
    return count[q] > threshold;
  }
};
